"""The index arithmetic of csrc/eegnet_fir_fft.hip, restated in numpy and checked on the CPU: the in-wave 1024-point FFT
(radix 16 x 16 x 4, 16 points per lane, one exchange through LDS slots and one by v_permlane32_swap / v_permlane16_swap
transposes between lanes and registers), the bank-conflict freedom of the LDS exchange under the MI355X lane-group rules
(ds_write_b64: groups of 16 lanes over 32 banks of 4 B, ds_read_b64: groups of 32 lanes over 64 banks), and the two
frequency-domain identities the kernels rest on (overlap-save correlation for the forward; the conjugate-product
accumulation for the weight gradient, with two electrodes packed into one complex signal).
Reference ops: nn.Conv2d(1, 8, (1, 300), padding='same') and its weight gradient - CNN_torch/EEGNet_tor.py:24,51,109."""
import numpy as np

N, LB, K = 1024, 704, 300
XP, WBUF = 66, 1056       # slot pitch of the LDS exchange, slots of a wave's buffer (eegnet_fir_fft.hip: fft1024)


def W(m):
    return np.exp(-2j * np.pi * (m % N) / N)


def dft4(a, inv):
    a0, a1, a2, a3 = a
    t0, t1, t2, t3 = a0 + a2, a0 - a2, a1 + a3, (a1 - a3) * (1j if inv else -1j)
    return [t0 + t2, t1 + t3, t0 - t2, t1 - t3]


def dft16(v, inv):
    y = [[None] * 4 for _ in range(4)]
    for b in range(4):
        r = dft4([v[b], v[4 + b], v[8 + b], v[12 + b]], inv)
        for c in range(4):
            w = np.exp(-2j * np.pi * (b * c) / 16)
            y[b][c] = r[c] * (np.conj(w) if inv else w)
    X = [None] * 16
    for c in range(4):
        r = dft4([y[0][c], y[1][c], y[2][c], y[3][c]], inv)
        for d in range(4):
            X[c + 4 * d] = r[d]
    return X


def swap32(a, b):
    """v_permlane32_swap on arrays of 64 lanes, in place: a[lanes 32-63] <-> b[lanes 0-31]."""
    t = a[32:].copy()
    a[32:] = b[:32]
    b[:32] = t


def swap16(a, b):
    """v_permlane16_swap, in place: a[lanes 16-31, 48-63] <-> b[lanes 0-15, 32-47]."""
    for lo in (0, 32):
        t = a[lo + 16:lo + 32].copy()
        a[lo + 16:lo + 32] = b[lo:lo + 16]
        b[lo:lo + 16] = t


def fft1024(x, inv=False):
    """Lane l holds x[l + 64 j] in register j on input and X[l + 64 j] on output - the kernel's layout."""
    regs = [[x[lane + 64 * j] for j in range(16)] for lane in range(64)]
    lds = np.zeros(WBUF, complex)
    for lane in range(64):
        regs[lane] = dft16(regs[lane], inv)
        for k1 in range(16):
            t = W(lane * k1)
            regs[lane][k1] *= np.conj(t) if inv else t
    for lane in range(64):
        for k1 in range(16):
            lds[XP * k1 + lane] = regs[lane][k1]
    for lane in range(64):
        regs[lane] = [lds[XP * (lane & 15) + (lane >> 4) + 4 * n2] for n2 in range(16)]
    for lane in range(64):
        regs[lane] = dft16(regs[lane], inv)
        for k2 in range(16):
            t = W(16 * (lane >> 4) * k2)
            regs[lane][k2] *= np.conj(t) if inv else t
    v = [np.array([regs[lane][k] for lane in range(64)]) for k in range(16)]      # v[register][lane]
    X = np.zeros(N, complex)
    for m in range(4):
        swap32(v[4 * m], v[4 * m + 2])
        swap32(v[4 * m + 1], v[4 * m + 3])
        swap16(v[4 * m], v[4 * m + 1])
        swap16(v[4 * m + 2], v[4 * m + 3])
        r = dft4(v[4 * m:4 * m + 4], inv)
        for k3 in range(4):                                                       # register m + 4 k3 of every lane
            X[np.arange(64) + 64 * (m + 4 * k3)] = r[k3]
    return X


def test_in_wave_fft_matches_numpy():
    rng = np.random.default_rng(0)
    x = rng.normal(size=N) + 1j * rng.normal(size=N)
    assert np.abs(fft1024(x) - np.fft.fft(x)).max() < 1e-11
    assert np.abs(fft1024(x, True) / N - np.fft.ifft(x)).max() < 1e-13


def _ways(slots, group, banks_in_slots):
    worst = 1
    for g in range(0, 64, group):
        s = [a % banks_in_slots for a in slots[g:g + group]]
        worst = max(worst, max(s.count(v) for v in set(s)))
    return worst


def test_lds_exchange_is_bank_conflict_free():
    # 8-byte slots: a ds_write_b64 group of 16 lanes covers 32 banks = 16 slots, a ds_read_b64 group of 32 lanes 64 banks = 32 slots
    for k in range(16):
        assert _ways([XP * k + lane for lane in range(64)], 16, 16) == 1
        assert _ways([XP * (lane & 15) + (lane >> 4) + 4 * k for lane in range(64)], 32, 32) == 1
    assert XP * 15 + 63 < WBUF                                       # the image fits the wave's exchange buffer


def test_overlap_save_identities():
    rng = np.random.default_rng(1)
    w = rng.normal(size=K)
    s = rng.normal(size=N) + 1j * rng.normal(size=N)                 # two electrodes packed: real + i imag
    H = np.conj(np.fft.fft(np.r_[w, np.zeros(N - K)])) / N
    y = fft1024(fft1024(s) * H, True)
    ref = np.array([np.dot(w, s[j:j + K]) for j in range(LB)])       # y[j] = sum_k w[k] s[j + k], no wrap for j < 704
    assert np.abs(y[:LB] - ref).max() < 1e-11
    assert LB + K - 1 <= N and N - LB + 1 == 321                     # the longest kernel the block length admits
    d = np.zeros(N, complex)
    d[:LB] = rng.normal(size=LB) + 1j * rng.normal(size=LB)          # dy of the two electrodes, zero-padded
    R = fft1024(fft1024(s) * np.conj(fft1024(d)), True) / N
    ref = np.array([np.dot(d[:LB].real, s[k:k + LB].real) + np.dot(d[:LB].imag, s[k:k + LB].imag) for k in range(K)])
    assert np.abs(R[:K].real - ref).max() < 1e-10                    # Re(.) = sum over BOTH electrodes of the pair
