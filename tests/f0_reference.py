"""The clip's f0 track restated in float64 numpy (own code, written from the published algorithm: D. Talkin, "A robust
algorithm for pitch tracking (RAPT)", 1995, with the defaults of its ``get_f0`` program): the contract of
animateportrait_amd/f0.py and csrc/seq/seq_f0.hip, and the reference of their tests.

One NCCF pass at the full rate (no decimated first pass), candidates by local maxima + parabola, a dynamic programme over the
candidates and the unvoiced hypothesis of every frame, ``speaker_normalization`` of the voiced log-f0.  Where the paper leaves a
detail open this file decides (DESIGN.md section 4e lists the decisions):
  * samples outside the signal read as zero BEFORE the reference window's mean is subtracted from the whole span;
  * the 19 kept candidates are the largest REFINED values (smaller lag first on a tie), and the refined lag and value enter
    every cost;
  * the Hann window of the rms / LPC frames is 0.5 - 0.5 cos(2 pi (i + 0.5) / 480), their rms is sqrt(sum (w x)^2 / 480);
  * the LPC autocorrelation gets r[0] <- r[0] (1 + 1e-7) + 1 (a white-noise floor of one unit on the 16-bit scale), which makes
    digital silence a frame like any other: I = 1, S = 1;
  * frame 0 has no predecessor: D_0 = d_0, and its table entries are S = 1, rr = 1;
  * states are ordered candidates by ascending lag, then the unvoiced hypothesis; every tie goes to the lowest index.

pysptk is absent from the build image, so parity of this file with ``sptk.rapt`` itself is unpinned."""
import numpy as np

FS = 16000
HOP = 256
N_CORR = 120                  # 0.0075 fs: the correlation window
N_LPC = 480                   # 0.03 fs: the rms / LPC window
LPC_ORDER = 18                # 2 + fs / 1000
N_CANDS = 19                  # get_f0's n_cands 20: 19 voiced hypotheses + the unvoiced one
CAND_THRESH = 0.3
LAG_WEIGHT = 0.3
FREQ_WEIGHT = 0.02
DOUBLE_COST = 0.35
TRANS_COST = 0.005
TRANS_AMP = 0.5
TRANS_SPEC = 0.5
VOICE_BIAS = 0.0
A_FLOOR = (100.0 * N_CORR) ** 2           # energy of amplitude-10 noise on the 16-bit scale, squared with n
UNVOICED = -1e10
LN2 = np.log(2.0)


def lag_range(gender):
    """(Kmin, Kmax) = (ceil(fs / hi), floor(fs / lo)): 'F' 100 .. 600 Hz, 'M' 50 .. 250 Hz"""
    lo, hi = {'F': (100, 600), 'M': (50, 250)}[gender]
    return -(-FS // hi), FS // lo


def frame_count(n_samples):
    return n_samples // HOP + 1


def tracker_input(wav):
    """``wav.astype(np.float32) * 32768`` as the reference hands it to rapt"""
    return np.asarray(wav).astype(np.float32) * np.float32(32768)


def _span(x, start, n):
    out = np.zeros(n)
    a, b = max(start, 0), min(start + n, x.shape[0])
    if b > a:
        out[a - start:b - start] = x[a:b]
    return out


def nccf(x, t, kmin, kmax):
    """phi(k) for k = kmin - 1 .. kmax + 1 of frame t (index 0 <-> k = kmin - 1)"""
    s = _span(x, HOP * t - N_CORR // 2, N_CORR + kmax + 2)
    s = s - s[:N_CORR].mean()
    ref = s[:N_CORR]
    e0 = float(np.dot(ref, ref))
    ks = np.arange(kmin - 1, kmax + 2)
    win = np.lib.stride_tricks.sliding_window_view(s, N_CORR)[ks]
    return (win @ ref) / np.sqrt(e0 * (win * win).sum(1) + A_FLOOR)


def pick_candidates(phi, kmin, kmax):
    """-> (lags, values) of at most 19 candidates, ascending lag; phi as nccf returns it"""
    k = np.arange(kmin, kmax + 1)
    a, b, c = phi[:-2], phi[1:-1], phi[2:]
    ok = (b > a) & (b >= c) & (b > 0) & (b >= CAND_THRESH * b.max())
    a, b, c, k = a[ok], b[ok], c[ok], k[ok]
    d = 0.5 * (a - c) / (a - 2.0 * b + c)
    lag, val = k + d, b - 0.25 * (a - c) * d
    keep = np.sort(np.lexsort((k, -val))[:N_CANDS])          # the largest values, smaller k first on a tie; then by lag
    return lag[keep], val[keep]


def hann_window():
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * (np.arange(N_LPC) + 0.5) / N_LPC)


def lpc_frame(x, t):
    """(r[0 .. 18] of the Hann-weighted frame centred on 256 t with the noise floor on r[0], its rms)"""
    f = _span(x, HOP * t - N_LPC // 2, N_LPC) * hann_window()
    r = np.array([np.dot(f[:N_LPC - m], f[m:]) for m in range(LPC_ORDER + 1)])
    rms = np.sqrt(r[0] / N_LPC)
    r[0] = r[0] * (1.0 + 1e-7) + 1.0
    return r, rms


def levinson(r):
    """autocorrelation method: (a[0 .. 18] with a[0] = 1, the residual energy)"""
    a = np.zeros(LPC_ORDER + 1)
    a[0] = 1.0
    err = r[0]
    for m in range(1, LPC_ORDER + 1):
        k = -(r[m] + np.dot(a[1:m], r[m - 1:0:-1])) / err
        prev = a.copy()
        a[m] = k
        a[1:m] = prev[1:m] + k * prev[m - 1:0:-1]
        err = err * (1.0 - k * k)
    return a, err


def itakura(r_cur, a_prev, err_cur):
    """distortion of the current frame (autocorrelation r_cur, own residual err_cur) under the previous frame's predictor"""
    b = np.array([np.dot(a_prev[:LPC_ORDER + 1 - m], a_prev[m:]) for m in range(LPC_ORDER + 1)])
    return max((r_cur[0] * b[0] + 2.0 * np.dot(r_cur[1:], b[1:])) / err_cur, 1.0)


def stationarity(x, n_frames):
    """(rr, S) per frame; frame 0: 1, 1"""
    rr, s = np.ones(n_frames), np.ones(n_frames)
    prev = None
    for t in range(n_frames):
        r, rms = lpc_frame(x, t)
        a, err = levinson(r)
        if prev is not None:
            rr[t] = (rms + 1.0) / (prev[1] + 1.0)
            s[t] = 0.2 / (itakura(r, prev[0], err) - 0.8)
        prev = (a, rms)
    return rr, s


def candidate_tables(x, gender='F', n_frames=None):
    """x: the tracker's input (16-bit scale).  -> dict: count (T,), lag (T, 19), val (T, 19) (zero behind count), rr (T,), s (T,),
    and phi (T, kmax - kmin + 3) for the tests' exclusions"""
    x = np.asarray(x, dtype=np.float64)
    kmin, kmax = lag_range(gender)
    T = frame_count(x.shape[0]) if n_frames is None else n_frames
    count = np.zeros(T, np.int32)
    lag, val = np.zeros((T, N_CANDS)), np.zeros((T, N_CANDS))
    phis = np.zeros((T, kmax - kmin + 3))
    for t in range(T):
        phis[t] = nccf(x, t, kmin, kmax)
        l, v = pick_candidates(phis[t], kmin, kmax)
        count[t] = len(l)
        lag[t, :len(l)], val[t, :len(l)] = l, v
    rr, s = stationarity(x, T)
    return {'count': count, 'lag': lag, 'val': val, 'rr': rr, 's': s, 'phi': phis, 'kmin': kmin, 'kmax': kmax}


def _two_smallest_gap(v):
    if len(v) < 2:
        return np.inf
    p = np.partition(v, 1)
    return float(p[1] - p[0])


def viterbi(tab, kmax):
    """The dynamic programme on candidate tables.  -> (path (T,) int: candidate index or -1 for unvoiced, margin (T,): the gap
    between the best and the second-best predecessor of the state chosen at t + 1 -- for the last frame between the two best
    terminal states --, i.e. how firmly frame t's state is decided)"""
    count, lag, val, rr, s = tab['count'], tab['lag'], tab['val'], tab['rr'], tab['s']
    T = len(count)
    back, gaps = [], []
    D = llag = None
    for t in range(T):
        n = int(count[t])
        c, l = np.asarray(val[t, :n], np.float64), np.asarray(lag[t, :n], np.float64)
        d = np.concatenate([1.0 - c * (1.0 - LAG_WEIGHT * l / kmax), [VOICE_BIAS + (c.max() if n else 0.0)]])
        ll = np.log(l)
        if t == 0:
            bp, gap, tot = np.zeros(n + 1, np.int64), np.full(n + 1, np.inf), d
        else:
            m = len(llag)
            delta = np.zeros((m + 1, n + 1))
            xi = ll[None, :] - llag[:, None]
            delta[:m, :n] = FREQ_WEIGHT * np.minimum(np.abs(xi), DOUBLE_COST + np.minimum(np.abs(xi - LN2), np.abs(xi + LN2)))
            delta[:m, n] = TRANS_COST + TRANS_SPEC * s[t] + TRANS_AMP * rr[t]
            delta[m, :n] = TRANS_COST + TRANS_SPEC * s[t] + TRANS_AMP / rr[t]
            tot = D[:, None] + delta
            bp = tot.argmin(0)                                      # the lowest index on a tie
            gap = np.array([_two_smallest_gap(tot[:, j]) for j in range(n + 1)])
            tot = d + tot.min(0)
        D = tot - tot.min()
        llag = ll
        back.append(bp)
        gaps.append(gap)
    path, margin = np.zeros(T, np.int64), np.zeros(T)
    j = int(D.argmin())
    margin[T - 1] = _two_smallest_gap(D)
    for t in range(T - 1, -1, -1):
        n = int(count[t])
        path[t] = j if j < n else -1
        if t > 0:
            margin[t - 1] = gaps[t][j]
            j = int(back[t][j])
    return path, margin


def log_f0(tab, path):
    lf = np.full(len(path), UNVOICED)
    v = path >= 0
    lf[v] = np.log(FS / np.asarray(tab['lag'], np.float64)[np.nonzero(v)[0], path[v]])
    return lf


def speaker_normalization(lf):
    """voiced -> (clip((v - mean) / std / 4, -1, 1) + 1) / 2 with the population std; no voiced frame: all stay -1e10; std = 0
    (the reference divides by zero in both cases): voiced frames get 0.5"""
    out = np.array(lf, dtype=np.float64)
    v = out != UNVOICED
    if not v.any():
        return out
    mean, std = out[v].mean(), out[v].std()
    out[v] = 0.5 if std == 0 else (np.clip((out[v] - mean) / std / 4.0, -1.0, 1.0) + 1.0) / 2.0
    return out


def harmonic_signal(freq, seed, n=FS, gap=None, amp=4000.0, noise=20.0):
    """The tests' synthetic voice: five harmonics 1 / h at ``amp`` (freq: Hz, a number or one value per sample) plus seeded
    noise; ``gap`` = (first, last + 1) samples of silence in the tone.  float32, on the 16-bit scale."""
    phase = 2.0 * np.pi * np.cumsum(np.broadcast_to(np.asarray(freq, dtype=np.float64), (n,))) / FS
    x = sum(amp / h * np.sin(h * phase) for h in range(1, 6)) if amp else np.zeros(n)
    if gap is not None:
        x[gap[0]:gap[1]] = 0.0
    return (x + noise * np.random.RandomState(seed).randn(n)).astype(np.float32)


def candidate_slack(phi, kmin, kmax, eps=1e-3, tiny=1e-9):
    """Every lag of a frame that is a candidate or close to being one: (k, lag, value, sure).  The zones: ``eps`` around the two
    thresholds (phi > 0, phi >= 0.3 max), as the tests' contract sets it; ``tiny`` around the two local-maximum conditions, which
    compare sums of the same 120 fp64 products taken in another order (their difference is below 120 x 2^-53 of the products'
    absolute sum over a denominator above 1.2e4: 1e-9 is generous).  sure: a candidate outside both zones."""
    k = np.arange(kmin, kmax + 1)
    a, b, c = phi[:-2], phi[1:-1], phi[2:]
    peak, thr = np.minimum(b - a, b - c), np.minimum(b, b - CAND_THRESH * b.max())
    near = (peak > -tiny) & (thr > -eps)
    sure = ((peak > tiny) & (thr > eps))[near]
    a, b, c, k = a[near], b[near], c[near], k[near]
    with np.errstate(divide='ignore', invalid='ignore'):
        d = 0.5 * (a - c) / (a - 2.0 * b + c)
    return k, k + d, b - 0.25 * (a - c) * d, sure


def f0_track(x, gender='F'):
    """x: the tracker's input.  -> dict: f0_norm (T,), log_f0, path, margin, and the tables"""
    tab = candidate_tables(x, gender)
    path, margin = viterbi(tab, tab['kmax'])
    lf = log_f0(tab, path)
    return dict(tab, path=path, margin=margin, log_f0=lf, f0_norm=speaker_normalization(lf))
