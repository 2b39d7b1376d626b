"""CPU restatement of the lazy replay's once-per-row range test (anirec_train_lazy.hpp, lz_bound / lz_entry_ok): the
L2-only Adam step in NumPy fp32 (every operation correctly rounded, as on the GPU), the entry test as the kernel
computes it, and, for every admitted element, the bounds the kernel's comment proves — checked step by step over
whole windows on operands drawn log-uniformly over many binades, most of them near the admission limits."""
import numpy as np

F32 = np.float32
C1, C2, EPS = F32(0.1), F32(0.001), F32(1e-7)


def _step(w, m, v, alpha, two_l2):
    g = w * two_l2
    mn = m + (g - m) * C1
    vn = v + (g * g - v) * C2
    num = mn * alpha
    den = np.sqrt(vn) + EPS
    return w - num / den, mn, vn, num


def _entry(w, m, v, alpha, two_l2):
    """lz_bound + lz_entry_ok for one element per lane (v_rsq_f32 restated as the correctly rounded 1 / sqrt)"""
    amax = alpha.max()
    k = F32(1.01) * abs(two_l2) * amax
    kv = C2 * two_l2 * two_l2
    with np.errstate(divide="ignore", over="ignore", invalid="ignore", under="ignore"):
        vb = np.maximum(v, kv * (w * w))         # the first step lifts v to at least c2 (2 lambda w)^2
        f = F32(1) + np.minimum(k * (F32(1) / np.sqrt(vb)), k * F32(1e7))
        f = f * f
        f = f * f
        f = f * f
        x0 = np.maximum(np.abs(m), abs(two_l2) * np.abs(w))
        xf = x0 * f
        ok = (vb >= F32(2.0 ** -95)) & (v <= F32(2.0 ** 95)) & (xf <= F32(2.0 ** 46)) & (xf * amax <= F32(2.0 ** 58))
    return ok, x0, f, vb


def _draw(rng, n, lo, hi):
    return (F32(2.0) ** rng.uniform(lo, hi, n).astype(F32)).astype(F32) * rng.choice([F32(-1), F32(1)], n)


def test_admitted_elements_stay_inside_the_short_sequences_range_for_a_whole_window():
    rng = np.random.default_rng(0)
    n = 400_000
    checked = 0
    for two_l2, lr_exp, zero_v in ((F32(2e-4), -17, False), (F32(2e-4), 8, False), (F32(0.5), -3, False),
                                   (F32(0.0), 10, False), (F32(3.0), 0, False), (F32(2e-4), -17, True),
                                   (F32(0.5), -3, True), (F32(3.0), 0, True)):
        alpha = (F32(2.0) ** rng.uniform(lr_exp - 2, lr_exp, 8).astype(F32)).astype(F32)
        w = _draw(rng, n, -40, 50)
        m = _draw(rng, n, -70, 50)
        v = np.abs(_draw(rng, n, -100, 100))
        if zero_v:
            v[: n // 2] = 0.0                                             # rows fresh from initialisation
            m[: n // 4] = 0.0
        ok, x0, f, vb = _entry(w, m, v, alpha, two_l2)
        assert ok.sum() > 1000 and (~ok).sum() > 1000
        if zero_v:
            assert ok[: n // 2].sum() > 1000
        w, m, v = w[ok], m[ok], v[ok]
        x0, f, vb = x0[ok], f[ok], vb[ok]
        with np.errstate(over="ignore", invalid="ignore", under="ignore"):
            for j in range(8):
                w, m, v, num = _step(w, m, v, alpha[j], two_l2)
                assert np.all(v >= F32(0.989) * vb)                       # (v lo), the first step's lift included
                assert np.all((v >= F32(2.0 ** -96)) & (v <= F32(2.0 ** 96)))
                assert np.all(np.abs(num) <= F32(2.0 ** 60))
                xj = np.maximum(np.abs(m), abs(two_l2) * np.abs(w))
                assert np.all(xj <= x0 * f * F32(1 + 2.0 ** -18))           # the growth bound X_j <= X_0 F
        checked += int(ok.sum())
    assert checked > 100_000


def test_fresh_rows_are_admitted():
    """v_0 = m_0 = 0 (the moments' initial values) with the S109M rates: the first step's lift admits the row"""
    rng = np.random.default_rng(2)
    w = rng.uniform(-0.05, 0.05, 100_000).astype(F32)
    z = np.zeros_like(w)
    alpha = (F32(1e-5) * np.sqrt(F32(1) - F32(0.999) ** np.arange(1, 9, dtype=F32))
             / (F32(1) - F32(0.9) ** np.arange(1, 9, dtype=F32))).astype(F32)
    ok = _entry(w, z, z, alpha, F32(2e-4))[0]
    assert ok[np.abs(w) > 1e-9].all()


def test_second_moment_lower_bound_is_tight_enough_for_the_factor_two_margin():
    """v_j >= v_0 (b2 (1 - 2^-23))^j >= 0.99 v_0 over 8 steps whatever g is; 2 x 0.99 > 1 keeps v_j above 2^-96"""
    rng = np.random.default_rng(1)
    v0 = (F32(2.0 ** -95) * (F32(1) + rng.random(100_000).astype(F32))).astype(F32)
    v = v0.copy()
    for _ in range(8):
        v = v + (F32(0) - v) * C2          # g = 0: the fastest decay
    assert np.all(v >= F32(0.99) * v0) and np.all(v > F32(2.0 ** -96))
    assert F32(0.999) ** 8 > F32(0.99)
