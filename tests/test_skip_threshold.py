"""THETA = 128 of the VolSDF renderer's skipping rule (csrc/volsdf_render.hip, SKIP_THETA): a ray whose fp32 running optical depth over the
intervals k < s has reached THETA is dead from sample s on - k_composite_volsdf's transmittance T_k is EXACTLY 0 for every k >= s, so the samples
behind s reach no output.  The kernel forms T as a product, not as exp(-sum): 3 intervals per lane (P = 192), the six levels of wave_excl_prod's
shuffle tree, then `T *= p` inside the lane; with denormals on, each multiplication may round a tiny value UP.  Emulated here in numpy float32 in
exactly that association, over sequences built to reach THETA as barely as possible - and with every factor pushed up one ulp as well, for expf's
own last-place error.  Host arithmetic only."""
import numpy as np

THETA = np.float32(128.0)
P = 192
NINT = P - 1
SEG = (NINT + 63) >> 6          # intervals per lane: 3
F = np.float32


def running_sum(x):
    """s[:, k] = fp32 sum of x[:, :k], added in ascending k (the kernel's chain); shape [N, NINT + 1]."""
    s = np.zeros((x.shape[0], NINT + 1), dtype=F)
    for k in range(NINT):
        s[:, k + 1] = s[:, k] + x[:, k]
    return s


def composite_T(p):
    """T[:, k] as k_composite_volsdf computes it from the factors p [N, NINT] (float32)."""
    n = p.shape[0]
    pad = np.ones((n, 64 * SEG), dtype=F)
    pad[:, :NINT] = p
    pad = pad.reshape(n, 64, SEG)
    lp = np.ones((n, 64), dtype=F)
    for j in range(SEG):                                # pass 1: lp *= p, in the lane's order
        lp = lp * pad[:, :, j]
    v = lp.copy()
    o = 1
    while o < 64:                                       # wave_excl_prod: if (lane >= o) v *= shfl_up(v, o)
        t = v.copy()
        t[:, o:] = v[:, :-o]
        v[:, o:] = v[:, o:] * t[:, o:]
        o <<= 1
    T = np.ones((n, 64), dtype=F)
    T[:, 1:] = v[:, :-1]                                # exclusive: lane 0 gets 1
    out = np.empty((n, 64, SEG), dtype=F)
    for j in range(SEG):                                # T_k, then T *= p
        out[:, :, j] = T
        T = T * pad[:, :, j]
    return out.reshape(n, 64 * SEG)[:, :NINT]


def check_dead(x, need_marked=True):
    x = np.ascontiguousarray(x, dtype=F)
    assert (x >= 0).all()
    s = running_sum(x)
    reached = s >= THETA                                # [N, NINT + 1]: dead from sample k on
    marked = reached.any(axis=1)
    if need_marked:
        assert marked.all(), "every sequence of this family is built to reach THETA"
    first = np.where(marked, reached.argmax(axis=1), NINT + 1)
    p = np.exp(-x).astype(F)
    # expf correctly rounded / one ulp high wherever it is not 0 (a factor whose exact value rounds to 0 - x above 103.97 - is taken as 0: the
    # device's expf returns 0 below -103.28)
    for factors in (p, np.where(p > 0, np.minimum(np.nextafter(p, F(2.0)), F(1.0)), p)):
        T = composite_T(factors)
        behind = np.arange(NINT)[None, :] >= first[:, None]
        assert (T[behind] == 0.0).all(), f"non-zero T behind the marked sample: max {T[behind].max():.3e}"
    return int(marked.sum())


def scaled_to(x, s_at, total):
    """x scaled so that its (float64) sum over k < s_at is `total`; everything behind s_at is kept (it can only lower T)."""
    x = np.asarray(x, dtype=np.float64)
    return (x * (total / x[:s_at].sum())).astype(F)


JUST_OVER = (128.0, 128.00002, 128.001, 128.5)


def test_all_equal():
    rows = [scaled_to(np.ones(NINT), s, t) for s in range(1, NINT + 1) for t in JUST_OVER]
    assert check_dead(np.stack(rows), need_marked=False) >= len(rows) // 2      # a sum a rounding below 128.0 simply marks one sample later


def test_ramps():
    k = np.arange(1, NINT + 1, dtype=np.float64)
    rows = []
    for shape in (k, k[::-1], k ** 2, 1.0 / k, np.sqrt(k)):
        for s in range(2, NINT + 1, 3):
            for t in JUST_OVER:
                rows.append(scaled_to(shape, s, t))
    assert check_dead(np.stack(rows), need_marked=False) >= len(rows) // 2


def test_one_factor_per_lane_just_above_one_half():
    """A first term carries T to the edge of the denormal range; then one factor per lane just above 0.5 (the others 1): every level of the
    product halves a denormal, the case in which round-to-nearest-even rounds UP by the largest relative amount."""
    rows = []
    for x_half in (0.6931, 0.69314, 0.693147, 0.69):
        for m in range(1, 64):
            for pos in range(SEG):
                x = np.zeros(NINT)
                x[0] = 128.0 - x_half * (m - 1) + 1e-4
                idx = np.arange(SEG + pos, NINT, SEG)
                x[idx] = x_half
                rows.append(x.astype(F))
    assert check_dead(np.stack(rows), need_marked=False) >= len(rows) // 2


def test_single_large_term():
    rows = []
    for j in range(NINT):
        for big in (128.0, 128.00002, 200.0, 1e4):
            x = np.zeros(NINT)
            x[j] = big
            rows.append(x.astype(F))
            y = np.full(NINT, 1e-3)
            y[j] = big
            rows.append(y.astype(F))
    check_dead(np.stack(rows))


def test_random_draws():
    rng = np.random.default_rng(0)
    n = 10000
    scale = np.exp(rng.uniform(np.log(0.05), np.log(60.0), size=(n, 1)))
    x = rng.exponential(1.0, size=(n, NINT)) * scale
    x[rng.random((n, NINT)) < 0.3] = 0.0                # empty space: p = 1 exactly
    # half of the rows: rescaled so that the sum reaches THETA as barely as the rounding allows at a random sample
    s_at = rng.integers(1, NINT + 1, size=n)
    for i in range(0, n, 2):
        if x[i, :s_at[i]].sum() > 0:
            x[i] = scaled_to(x[i], s_at[i], 128.0 + rng.choice([0.0, 2e-5, 1e-3]))
    assert check_dead(x.astype(F), need_marked=False) >= n // 2


def test_not_vacuous_a_sum_of_100_leaves_light():
    """The emulation can tell: at a running sum of 100 the composite's T is still a non-zero (denormal) number."""
    rows = [scaled_to(np.ones(NINT), s, 100.0) for s in (1, 7, 64, 150, NINT)]
    x = np.stack(rows)
    s = running_sum(x)
    T = composite_T(np.exp(-x).astype(F))
    for i, s_at in enumerate((1, 7, 64, 150, NINT)):
        assert 99.9 < s[i, s_at] < 100.1
    assert (T[np.arange(3), [1, 7, 64]] > 0.0).all(), "e^-100 = 3.7e-44 is representable: nothing may be skipped there"
    assert (s[:, :-1][T == 0.0] > 100.0).all()
