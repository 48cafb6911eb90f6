"""eav_amd.optim._merge_rows - the one rule for "merge what is adjacent" - against the three loops it replaced
(tests/optim_merge_ref.py, kept word for word), on synthetic integer pointers; and the split of the criteria into
eav_amd/criteria.py with the old import path alive.  Host arithmetic only."""
import os
import random
import re

from tests import optim_merge_ref as R

BASES = (0x7F0000000000, 0x7F1000000000, 0x7F2000000000, 0x7F3000000000)     # p, g, m, v: four buffers, one layout
FLAT = [7, 64, 1, 4097, 300]


def layout(sizes, gaps=None, pads=None):
    """[(byte offset, numel, pad floats)]: tensor i + 1 begins gaps[i] bytes after the end of tensor i.  Default gaps: what
    flatten_parameters leaves, every tensor on a 16-byte boundary."""
    gaps = [-4 * n % 16 for n in sizes] if gaps is None else gaps
    pads = [0] * len(sizes) if pads is None else pads
    out, at = [], 0
    for n, gap, pad in zip(sizes, gaps, pads):
        out.append((at, n, pad))
        at += 4 * n + gap
    return out


def both(tensors, keys=None, shift=None, loose=False):
    """`tensors` (layout's rows) through _merge_rows and through every reference loop that takes them; returns the merged
    four-pointer rows as (ptrs, numel, slack, key).  keys: (step, lr, wd) per tensor.  shift: {(tensor, pointer): bytes}
    moves one pointer of one tensor.  loose: tensors outside a flat buffer (slack 1, two pointers only)."""
    from eav_amd.optim import _merge_rows
    keys = [(1, 1e-3, 0.01)] * len(tensors) if keys is None else keys
    shift = shift or {}
    ptrs = [tuple(BASES[k] + off + shift.get((i, k), 0) for k in range(4)) for i, (off, _, _) in enumerate(tensors)]
    slack = [1 if loose else 16 + 4 * pad for _, _, pad in tensors]
    numel = [n for _, n, _ in tensors]
    idx = range(len(tensors))

    def run(nptr, key):
        """_merge_rows over the first nptr pointers; its rows as (absolute pointers, numel, slack, key)."""
        rows = [[ptrs[i][0], tuple(p - ptrs[i][0] for p in ptrs[i][1:nptr]), numel[i], slack[i], key(i)] for i in idx]
        return [(tuple([at] + [at + d for d in rel]), n, s, k) for at, rel, n, s, k in _merge_rows(rows)]

    # accumulate() / clip_grad_norm_: two pointers, no key
    got = run(2, lambda i: None)
    want = R.merge_ranges([[ptrs[i][0], ptrs[i][1], numel[i], slack[i]] for i in idx])
    assert [[*p, n, s] for p, n, s, _ in got] == want and all(k is None for _, _, _, k in got)
    if loose:
        return got

    # the default step: four pointers, keyed by the step count
    got = run(4, lambda i: keys[i][0])
    want = R.merge_default([[*ptrs[i], numel[i], keys[i][0], None, slack[i] - 16] for i in idx])
    assert [[*p, n, k, None, s - 16] for p, n, s, k in got] == want

    # the table step: four pointers, keyed by (step, lr, weight decay)
    got = run(4, lambda i: keys[i])
    want = R.merge_jobs([[*ptrs[i], numel[i], *keys[i], slack[i] - 16] for i in idx])
    assert [[*p, n, *k, s - 16] for p, n, s, k in got] == want
    return got


def test_flat_layout_is_one_run_under_one_key_and_five_under_alternating_keys():
    t = layout(FLAT)
    assert [b[0] - (a[0] + 4 * a[1]) for a, b in zip(t, t[1:])] == [4, 0, 12, 12]
    (ptrs, numel, slack, key), = both(t)
    assert ptrs == BASES and numel == t[-1][0] // 4 + 300 and slack == 16 and key == (1, 1e-3, 0.01)
    for k in range(3):                                  # the neighbours differ in step, in lr or in weight decay only
        other = [1, 1e-3, 0.01]
        other[k] *= 2
        keys = [(1, 1e-3, 0.01) if i % 2 == 0 else tuple(other) for i in range(5)]
        assert [r[1] for r in both(t, keys)] == FLAT
    assert both(list(reversed(t))) == both(t)           # the input order does not matter
    assert both([]) == []
    assert both(t[:1]) == [(BASES, 7, 16, (1, 1e-3, 0.01))]


def test_the_slack_is_exclusive_and_the_joined_row_takes_the_joiners():
    assert len(both(layout([8, 8], gaps=[16, 0]))) == 2                     # 16 bytes at pad 0: not adjacent
    (_, numel, slack, _), = both(layout([8, 8], gaps=[16, 0], pads=[4, 0])) # slack 32 declared: joins ...
    assert numel == 8 + 4 + 8 and slack == 16                               # ... and carries the joiner's slack on
    assert len(both(layout([8, 8, 8], gaps=[16, 16, 0], pads=[4, 0, 0]))) == 2   # so the third tensor stays apart
    assert len(both(layout([8, 8], gaps=[32, 0], pads=[4, 0]))) == 2        # 16 + pad exactly: not adjacent
    assert len(both(layout([8, 8], gaps=[28, 0], pads=[4, 0]))) == 1
    assert len(both(layout([8, 8], gaps=[-4, 0]))) == 2                     # overlap: never merged
    assert len(both(layout([5, 8], gaps=[0, 0]), loose=True)) == 1          # loose tensors: exactly adjacent only
    assert len(both(layout([5, 8], gaps=[4, 0]), loose=True)) == 2


def test_every_pointer_must_sit_at_the_same_offset():
    t = layout([8, 8])
    assert len(both(t)) == 1
    for k in (1, 2, 3):                                 # g, m or v of the second tensor 4 bytes off, either way
        for by in (4, -4):
            assert len(both(t, shift={(1, k): by})) == 2


def test_random_layouts_against_all_three_loops():
    rng = random.Random(20240607)
    for _ in range(200):
        n = rng.randint(1, 40)
        sizes = [rng.choice((1, 3, 4, 7, 64, 300, 4097)) for _ in range(n)]
        gaps = [rng.choice((0, 4, 12, 16, 20, 32)) for _ in range(n)]
        pads = [rng.choice((0, 4, 8)) for _ in range(n)]
        distinct = [(rng.randint(1, 3), rng.choice((1e-3, 2.5e-4)), rng.choice((0.0, 0.01))) for _ in range(rng.randint(1, 3))]
        keys = [rng.choice(distinct) for _ in range(n)]
        order = list(range(n))
        rng.shuffle(order)
        t = layout(sizes, gaps, pads)
        merged = both([t[i] for i in order], [keys[i] for i in order])
        assert sum(r[1] for r in merged) >= sum(sizes) and len(merged) <= n
        both([t[i] for i in order], loose=True)


def test_criteria_moved_and_the_old_import_path_hands_out_the_same_objects():
    import eav_amd.criteria as C
    import eav_amd.optim as O
    for name in ("CrossEntropyLoss", "BCEWithLogitsLoss", "MSELoss", "unit_gradient", "head_is_wide", "HEAD_NARROW_CLASSES"):
        assert getattr(O, name) is getattr(C, name), name
    with open(os.path.join(os.path.dirname(C.__file__), "criteria.py")) as f:
        src = f.read()
    assert re.findall(r"^\s*from\s+(\.\S*|eav_amd\S*)\s+import\s+(.+)$", src, flags=re.M) == [(".", "_lib")]
    assert not re.search(r"^\s*import\s+eav_amd", src, flags=re.M)
