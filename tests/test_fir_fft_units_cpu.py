"""Unit list and forward deal of the FFT FIR kernels (csrc/eegnet_fir_fft.hip, `Units`), restated in numpy from their
definition: rows of S samples in blocks of 704, a tail of Lt = S - 704 (nblk - 1) outputs that shares a 1024-point
transform with another tail iff Lt + K - 1 <= 512; main units first, packed tails (2 p, 2 p + 1 of the flattened
sample x pair index) behind them.  Forward: up to 256 workgroups of 12 waves, nunits // nwaves full rounds, extra e to
workgroup e % nWG, wave slot e // nWG; wave slot w sits on SIMD w % 4.  Weight gradient: groups of 8 units of one kind,
the smallest grid that needs no more rounds than 256 workgroups would.  No GPU needed; one test compares the restatement
with eav_eegnet_fir_fft_plan, the rule as the launchers apply it."""
import numpy as np
import pytest

LB, NF, NWF = 704, 1024, 12
BENCH = (64, 30, 10000, 300)
SHAPES = [BENCH, (1, 2, 705, 300), (2, 3, 705, 300), (3, 1, 1409, 321), (2, 4, 917, 300), (2, 4, 918, 300),
          (2, 4, 896, 321), (2, 4, 897, 321), (1, 3, 1100, 64), (4, 30, 1500, 300), (2, 30, 500, 300), (2, 5, 704, 300)]


def units(B, C, S, K):
    """-> (list of units, packs); a unit is a list of (sample, pair, block, first slot of its half)"""
    npair, nblk = (C + 1) // 2, -(-S // LB)
    lt = S - (nblk - 1) * LB
    packs = lt + K - 1 <= NF // 2
    nmb = nblk - 1 if packs else nblk
    out = [[(b, pr, blk, 0)] for b in range(B) for pr in range(npair) for blk in range(nmb)]
    if packs:
        tails = [(b, pr) for b in range(B) for pr in range(npair)]
        for p in range((len(tails) + 1) // 2):
            out.append([(*t, nblk - 1, 512 * h) for h, t in enumerate(tails[2 * p:2 * p + 2])])
    return out, packs


def fwd_deal(nunits):
    """units per (workgroup, SIMD)"""
    nwg = min(256, max(1, -(-nunits // NWF)))
    nwaves = nwg * NWF
    rounds, extras = divmod(nunits, nwaves)
    per_simd = np.full((nwg, 4), rounds * (NWF // 4))
    seen = np.zeros(nunits, int)
    for r in range(rounds):
        seen[r * nwaves:(r + 1) * nwaves] += 1
    for e in range(extras):
        wg, slot = e % nwg, e // nwg
        assert slot < NWF
        per_simd[wg, slot % 4] += 1
        seen[rounds * nwaves + e] += 1
    assert (seen == 1).all()
    return per_simd


def wgrad_rounds(nmain, npk):
    groups = -(-nmain // 8) + -(-npk // 8)
    if groups <= 256:
        return max(1, groups), 1
    rounds = -(-groups // 256)
    return -(-groups // rounds), rounds


@pytest.mark.parametrize("B,C,S,K", SHAPES)
def test_every_block_is_covered_once_and_halves_do_not_overlap(B, C, S, K):
    us, packs = units(B, C, S, K)
    npair, nblk = (C + 1) // 2, -(-S // LB)
    lt = S - (nblk - 1) * LB
    seen = np.zeros((B, npair, nblk), int)
    for u in us:
        assert len(u) in (1, 2)
        for b, pr, blk, slot in u:
            seen[b, pr, blk] += 1
            if packs and blk == nblk - 1:
                # a packed half: its outputs j < Lt read slots j .. j + K - 1 of its own 512
                assert slot in (0, 512) and lt + K - 1 <= 512
            else:
                # an ordinary unit; in a packed list all of them are whole blocks
                assert len(u) == 1 and slot == 0 and (not packs or (blk + 1) * LB <= S)
    assert (seen == 1).all()
    # whatever the deal of the forward, every unit is run once
    fwd_deal(len(us))


@pytest.mark.parametrize("B,C,S,K", SHAPES)
def test_restatement_is_the_rule_the_launchers_use(B, C, S, K):
    """eav_eegnet_fir_fft_plan fills its fields from the functions the launchers call: the numpy restatement above must
    give the same unit list and the same two grids"""
    import ctypes
    from eav_amd import _lib
    out = (ctypes.c_int * 9)()
    _lib.call("eav_eegnet_fir_fft_plan", B, C, S, K, out)
    npair, nmb, nmain, ntail, npk, t0t, fwd_wgs, groups, wg_wgs = out
    us, packs = units(B, C, S, K)
    nblk = -(-S // LB)
    assert (npair, nmb) == ((C + 1) // 2, nblk - 1 if packs else nblk) and t0t == nmb * LB
    assert nmain == sum(1 for u in us if len(u) == 1 and u[0][3] == 0 and u[0][2] < nmb)
    assert ntail == (B * npair if packs else 0) and npk == len(us) - nmain == (ntail + 1) // 2
    assert fwd_wgs == fwd_deal(len(us)).shape[0]
    assert groups == -(-nmain // 8) + -(-npk // 8) and wg_wgs == wgrad_rounds(nmain, npk)[0]


def test_packing_condition_at_its_edges():
    assert units(2, 4, 917, 300)[1] and not units(2, 4, 918, 300)[1]
    assert units(2, 4, 896, 321)[1] and not units(2, 4, 897, 321)[1]
    assert units(1, 3, 1100, 64)[1] and not units(1, 3, 1100, 300)[1]
    assert not units(2, 30, 500, 300)[1] and not units(2, 5, 704, 300)[1]


def test_bench_shape_counts():
    us, packs = units(*BENCH)
    assert packs and len(us) == 13920
    nmain = sum(1 for u in us if u[0][3] == 0 and u[0][2] < 14)
    assert nmain == 13440 and len(us) - nmain == 480
    assert all(len(u) == 2 for u in us[nmain:])
    per_simd = fwd_deal(len(us))
    assert per_simd.shape == (256, 4) and per_simd.max() == 14 and per_simd.sum() == 13920
    # unpacked, the same row costs a fifteenth unit on some SIMD whatever the deal: 14400 > 14 x 1024
    assert len(units(64, 30, 10000, NF)[0]) == 14400 > 14 * 1024
    grid, rounds = wgrad_rounds(nmain, len(us) - nmain)
    assert (grid, rounds) == (249, 7)
    assert wgrad_rounds(14400, 0) == (225, 8)
