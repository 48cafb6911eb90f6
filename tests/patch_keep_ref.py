"""Host-only numpy restatements of csrc/patch_keep.hip (patch dropout of the AST / ViT encoders), written independently of
eav_amd.patch_keep: the plan of who is kept, its inverse table, and the three gather kernels in float64.

The hash is the generator of csrc/eav_common.h (eav_hash32) in the uint64 arithmetic of tests/encoder_dropout_kernel_ref.py's
hash_keep; here the 24-bit value itself is the key.  The key of patch p of sample b is hash32(seed + 2 counter, b P + p); the
kept set is the K smallest of the total order (key, p), listed ascending by p."""
import numpy as np

from tests.encoder_dropout_kernel_ref import M64

PATCH_KEEP_SITE = 1 << 23                          # encoder_dropout.SITES["patch_keep"]

# (B, P, K) of the plan cases: the smallest grid, one of two, half of ViT's 196, one dropped / none dropped of 300, half of
# AST's 1212, and the largest legal grid (2046 composite keys)
PLAN_CASES = [(1, 1, 1), (2, 2, 1), (3, 196, 98), (3, 300, 299), (2, 300, 300), (2, 1212, 606), (4, 2046, 1023)]
PLAN_COUNTERS = [1, 77]


# The model cases of tests/golden/patch_dropout*.npz (make_goldens_patch_dropout.py) and tests/test_patch_dropout_gpu.py, B = 3:
# name -> model kind, its reduced configuration, native frames / image, the input's frames / side, P, K, a rate p with
# keep_count(P, p) == K, which gradients are stored, and the file.  The keep tables are plan(B, P, K, plan_seed(SEED), COUNTER).
REDUCED = dict(hidden=64, layers=2, heads=4, ff=128)
WIDE = dict(hidden=128, layers=2, heads=2, ff=256)         # head_dim 64: the fused attention kernels
MODEL_CASES = {
    "vit64": dict(kind="vit", kw=REDUCED, native=64, size=64, P=16, K=7, p=0.55, grads="all", file="patch_dropout.npz"),
    "ast96": dict(kind="ast", kw=REDUCED, native=256, size=96, P=108, K=54, p=0.5, grads="all", file="patch_dropout.npz"),
    "ast256": dict(kind="ast", kw=REDUCED, native=256, size=256, P=300, K=150, p=0.5, grads="all",
                   file="patch_dropout_256.npz"),
    "ast256w": dict(kind="ast", kw=WIDE, native=256, size=256, P=300, K=107, p=0.643, grads="embeddings",
                    file="patch_dropout_256.npz"),
}
MODEL_B, MODEL_SEED, MODEL_COUNTER, MODEL_WSEED, MODEL_XSEED, MODEL_STD = 3, 20221, 5, 31, 310, 0.08


def model_keep(name):
    c = MODEL_CASES[name]
    assert keep_count(c["P"], c["p"]) == c["K"], name
    return plan(MODEL_B, c["P"], c["K"], plan_seed(MODEL_SEED), MODEL_COUNTER)[0]


def model_batch(name):
    """(inputs, labels) of a model case from the repository's seeded generators."""
    from eav_amd import synth
    c = MODEL_CASES[name]
    seed = MODEL_XSEED + c["size"] + c["kw"]["hidden"]
    if c["kind"] == "ast":
        return synth.mel_batch(seed, MODEL_B, c["size"], 128)
    return synth.frame_batch(seed, MODEL_B, c["size"])


def plan_seed(seed):
    """encoder_dropout.site_seed(seed, PATCH_KEEP_SITE)."""
    return (int(seed) + ((PATCH_KEEP_SITE + 1) << 40)) & M64


def keep_count(P, p):
    """timm.layers.PatchDropout: max(1, int(L * (1 - prob)))."""
    return max(1, int(P * (1.0 - p)))


def hash32(seed, n, counter=None):
    """eav_hash32(seed', idx) for idx = 0 .. n-1, seed' = seed + 2 counter (mod 2^64): uint32 [n], 24 random bits."""
    seed = (int(seed) + (0 if counter is None else 2 * int(counter))) & M64
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return (z >> np.uint64(40)).astype(np.uint32)


def plan(B, P, K, seed, counter=None, keys=None):
    """(keep int32 [B, K], inv int32 [B, P]); keys: explicit uint32 [B, P] instead of the hash."""
    key = hash32(seed, B * P, counter).reshape(B, P) if keys is None else np.asarray(keys, np.uint32).reshape(B, P)
    keep = np.empty((B, K), np.int32)
    for b in range(B):
        order = sorted(range(P), key=lambda p: (int(key[b, p]), p))       # the total order, spelled out
        keep[b] = sorted(order[:K])
    return keep, invert(keep, P)


def tie_cases(P, K):
    """[(name, keys uint32 [1, P], the kept patches)] with ties the hash gives with probability ~2^-24 only; P >= K + 2.
    The expected sets are written down from the rule, not computed by plan()."""
    assert P >= K + 2
    equal = np.full((1, P), 7, np.uint32)
    front = np.full((1, P), 200, np.uint32)            # K - 1 small keys in front, patches K-1 and K tie for the last place
    front[0, :K - 1], front[0, K - 1:K + 1] = 1, 5
    back = np.full((1, P), 200, np.uint32)             # the same keys in the other index order: the small ones at the end
    back[0, P - K + 1:], back[0, P - K - 1:P - K + 1] = 1, 5
    spread = np.full((1, P), 200, np.uint32)           # the tied pair apart, small keys on both sides of it
    pair = [0, 2]
    lows = [p for p in range(P) if p not in pair][:K - 1]
    spread[0, lows], spread[0, pair] = 1, 5
    down = np.arange(P, 0, -1, dtype=np.uint32)[None]
    return [("equal", equal, np.arange(K)), ("tie at K-1 / K", front, np.arange(K)),
            ("tie, reversed", back, np.array([P - K - 1] + list(range(P - K + 1, P)))),
            ("tie, spread", spread, np.array(sorted(lows + pair[:1]))), ("descending", down, np.arange(P - K, P))]


def invert(keep, P):
    keep = np.asarray(keep)
    inv = np.full((keep.shape[0], P), -1, np.int32)
    for b in range(keep.shape[0]):
        for s, p in enumerate(keep[b]):
            inv[b, p] = s
    return inv


def gather_rows(full, keep):
    """full [B, P, ...] -> [B, K, ...]: row (b, s) is full[b, keep[b, s]]."""
    return np.stack([full[b][np.asarray(keep[b])] for b in range(full.shape[0])])


def embed_finish_keep_ref(h, cls, dist, pos, keep, nextra):
    """h [B, nextra + K, D] with the projected kept patches in rows nextra.., pos [nextra + P, D] -> float64."""
    out = np.asarray(h, np.float64).copy()
    pos = np.asarray(pos, np.float64)
    out[:, 0] = np.asarray(cls, np.float64) + pos[0]
    if nextra == 2:
        out[:, 1] = np.asarray(dist, np.float64) + pos[1]
    for b in range(out.shape[0]):
        out[b, nextra:] += pos[nextra + np.asarray(keep[b])]
    return out


def embed_bwd_keep_ref(dh, inv, nextra):
    """dh [B, nextra + K, D], inv [B, P] -> (dpos float64 [nextra + P, D], sum |dh| of the same terms, demb [B K, D])."""
    dh = np.asarray(dh, np.float64)
    B, _, D = dh.shape
    P = inv.shape[1]
    dpos, mag = np.zeros((nextra + P, D)), np.zeros((nextra + P, D))
    dpos[:nextra], mag[:nextra] = dh[:, :nextra].sum(0), np.abs(dh[:, :nextra]).sum(0)
    for b in range(B):
        for p in range(P):
            if inv[b, p] >= 0:
                dpos[nextra + p] += dh[b, nextra + inv[b, p]]
                mag[nextra + p] += np.abs(dh[b, nextra + inv[b, p]])
    return dpos, mag, dh[:, nextra:].reshape(-1, D)
