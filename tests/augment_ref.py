"""NumPy restatement of eav_augment_gather (csrc/augment.hip, the contract in include/eav_hip.h) in float64, and a builder
of table records.  Shared by the kernel test and the trainer tests, which replay BatchAugment.plan_epoch's table."""
import numpy as np

RECORD_INTS = 12


def record(i, j, lam, flip=False, rows=((0, 0), (0, 0)), cols=((0, 0), (0, 0))):
    """One table record: source, partner, the bits of the fp32 lambda, flip, two row bands, two column bands."""
    bits = int(np.array([lam], dtype=np.float32).view(np.int32)[0])
    return [int(i), int(j), bits, int(bool(flip)), rows[0][0], rows[0][1], rows[1][0], rows[1][1],
            cols[0][0], cols[0][1], cols[1][0], cols[1][1]]


def lam_of(table):
    return np.ascontiguousarray(table[:, 2]).view(np.float32)


def gather(x, table, fill):
    """x [N, R, C] -> (out float64 [B, R, C], masked bool [B, R, C], mag float64 [B, R, C]) with
    out = fill inside any band, else lam x[i, r, c'] + (1 - lam) x[j, r, c'] (c' mirrored under a flip) evaluated in float64
    from the fp32 lambda, and mag = lam |a| + (1 - lam) |b|, the scale of the fp32 rounding bound.  A record with
    lam == 1 takes the source alone: a NaN in its partner does not show."""
    x = np.asarray(x)
    N, R, C = x.shape
    B = table.shape[0]
    out = np.empty((B, R, C), dtype=np.float64)
    masked = np.zeros((B, R, C), dtype=bool)
    mag = np.zeros((B, R, C), dtype=np.float64)
    lams = lam_of(table).astype(np.float64)
    rr, cc = np.arange(R)[:, None], np.arange(C)[None, :]
    for b in range(B):
        q = table[b]
        a, p = x[q[0]].astype(np.float64), x[q[1]].astype(np.float64)
        if q[3]:
            a, p = a[:, ::-1], p[:, ::-1]
        lam = lams[b]
        if lam == 1.0:
            out[b], mag[b] = a, np.abs(a)
        else:
            out[b] = lam * a + (1.0 - lam) * p
            mag[b] = lam * np.abs(a) + (1.0 - lam) * np.abs(p)
        m = ((rr >= q[4]) & (rr < q[5])) | ((rr >= q[6]) & (rr < q[7])) | ((cc >= q[8]) & (cc < q[9])) | \
            ((cc >= q[10]) & (cc < q[11]))
        masked[b] = m
        out[b][m] = fill
    return out, masked, mag


def soft_targets(y, table, NC):
    """lam onehot(y[i]) + (1 - lam) onehot(y[j]) in float64, exactly 1 where the labels coincide."""
    B = table.shape[0]
    t = np.zeros((B, NC), dtype=np.float64)
    lams = lam_of(table).astype(np.float64)
    for b in range(B):
        yi, yj = int(y[table[b, 0]]), int(y[table[b, 1]])
        if yi == yj:
            t[b, yi] = 1.0
        else:
            t[b, yi], t[b, yj] = lams[b], 1.0 - lams[b]
    return t
