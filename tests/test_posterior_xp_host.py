"""CPU: the extended-precision posterior reference of tests/_posterior_xp.py, held honest without a GPU.

  a. ``reference`` (np.longdouble) against an independent 50-digit mpmath evaluation of the same contract;
  b. every case of the table is in the regime it is meant to cover (ill-conditioned state, near-data candidates
     whose σ² is far below the older suites' absolute tolerance, far candidates whose kernel values vanish);
  c. the fp64 restatement — the yardstick the device bar is 4× of — stays within 8 roundings of the reference.
     This is a condition on the generator, not a measurement: if a change to the generator breaks it, the generator
     is what gets fixed.
"""
import numpy as np
import pytest

import _posterior_xp as xp

ALL = [(n, d, k) for n, d in xp.CASES for k in xp.KERNELS]
ids = lambda c: f"n{c[0]}-d{c[1]}-{c[2]}"  # noqa: E731


# ----------------------------------------------------------------------------- a. helper against mpmath
def _mp_reference(st, Xc, kernel, cols):
    import mpmath as mp
    mp.mp.dps = 50
    f = lambda a: [mp.mpf(float(v)) for v in a]  # noqa: E731
    X = [f(row) for row in st.X]
    ls, alpha, sf2 = f(st.lengthscale), f(np.asarray(st.alpha).reshape(-1)), mp.mpf(float(st.variance))
    Linv = [f(row) for row in st.Linv]
    n, s5 = len(X), mp.sqrt(5)
    mus, vars_ = [], []
    for j in cols:
        x = f(Xc[j])
        k = []
        for i in range(n):
            r2 = mp.fsum(((xj - Xij) / lj) ** 2 for xj, Xij, lj in zip(x, X[i], ls))
            if kernel == "matern52":
                r = mp.sqrt(r2)
                k.append(sf2 * (1 + s5 * r + mp.mpf(5) / 3 * r2) * mp.exp(-s5 * r))
            else:
                k.append(sf2 * mp.exp(-r2 / 2))
        mus.append(mp.fsum(a * ki for a, ki in zip(alpha, k)))
        v = [mp.fsum(Linv[i][c] * k[c] for c in range(i + 1)) for i in range(n)]
        vars_.append(sf2 - mp.fsum(vi * vi for vi in v))
    return mus, vars_


@pytest.mark.parametrize("kernel", xp.KERNELS)
@pytest.mark.parametrize("n,d", [(20, 2), (50, 4)])
def test_reference_matches_mpmath(n, d, kernel):
    import mpmath as mp
    st, Xc, (mu, var, _, _), (s_mu, s_var) = xp.case(n, d, kernel)
    cols = list(range(0, xp.N_CAND, 5))
    mus, vars_ = _mp_reference(st, Xc, kernel, cols)
    worst_mu = worst_var = 0.0
    for j, m, v in zip(cols, mus, vars_):
        # a longdouble converts to mpmath exactly as the sum of its fp64 head and tail
        ld = lambda z: mp.mpf(float(z)) + mp.mpf(float(z - np.longdouble(float(z))))  # noqa: E731
        worst_mu = max(worst_mu, float(abs(ld(mu[j]) - m) / (mp.mpf(xp.U) * ld(s_mu[j]))))
        worst_var = max(worst_var, float(abs(ld(var[j]) - v) / (mp.mpf(xp.U) * ld(s_var[j]))))
    print(f"n={n} d={d} {kernel}: |longdouble - mpmath| / (u S): mu {worst_mu:.2e} var {worst_var:.2e}")
    assert worst_mu <= 1e-3 and worst_var <= 1e-3


# ----------------------------------------------------------------------------- b. the regime
@pytest.mark.parametrize("case", ALL, ids=ids)
def test_case_is_in_the_regime(case):
    n, d, kernel = case
    st, Xc, (mu, var, _, _), _ = xp.case(n, d, kernel)
    sf2 = np.longdouble(st.variance)
    linv = np.abs(st.Linv).max()
    smallest = float(var[:16].min() / sf2)
    far_mu = float(np.abs(mu[xp.FAR]).max() / np.abs(st.alpha).sum())
    print(f"n={n} d={d} {kernel}: max|Linv| {linv:.2e}  min var / sf2 {smallest:.2e}  far |mu| / sum|alpha| {far_mu:.1e}")
    assert linv >= 5e2
    assert smallest <= 1e-8
    assert np.all(var[xp.FAR] == sf2)
    assert far_mu <= 1e-100


def test_candidate_groups():
    st, Xc, _, _ = xp.case(20, 2, "matern52")
    assert Xc.shape == (xp.N_CAND, 2) and xp.GROUPS[-1][2] == xp.N_CAND
    assert np.array_equal(Xc[:4], st.X[:4]) and np.array_equal(Xc[4:8], st.X[-4:])
    assert np.array_equal(Xc[8:12], st.X[-4:] + 1e-6) and np.array_equal(Xc[12:16], st.X[-4:] + 1e-9)
    r = (Xc[xp.RAY, 0] - st.X[0, 0]) / st.lengthscale[0] * np.sqrt(5.0)
    np.testing.assert_allclose(r, [600.0, 700.0, 740.0, 760.0], rtol=1e-12)
    assert np.array_equal(Xc[xp.RAY, 1], np.repeat(st.X[0, 1], 4))
    # both objectives share rows, hyperparameters and candidates
    st1, Xc1, _, _ = xp.case(20, 2, "matern52", 1)
    assert np.array_equal(st1.X, st.X) and np.array_equal(st1.lengthscale, st.lengthscale) and np.array_equal(Xc1, Xc)
    assert not np.array_equal(st1.alpha, st.alpha)


# ----------------------------------------------------------------------------- c. cap on the yardstick
def test_restatement_stays_within_the_cap():
    worst_mu = worst_var = 0.0
    for n, d, kernel in ALL:
        e_mu, e_var = xp.restatement_error(n, d, kernel)
        print(f"n={n} d={d} {kernel}: restatement e_mu {e_mu:.2f} e_var {e_var:.2f}")
        worst_mu, worst_var = max(worst_mu, e_mu), max(worst_var, e_var)
    t_mu, t_var = xp.bar()
    print(f"worst restatement e: mu {worst_mu:.2f} var {worst_var:.2f}   bar T = 4 x worst: mu {t_mu:.2f} var {t_var:.2f}")
    assert worst_mu <= 8.0 and worst_var <= 8.0
    assert (t_mu, t_var) == (4.0 * worst_mu, 4.0 * worst_var)


def test_ceiling_is_above_the_bar():
    t_mu, t_var = xp.bar()
    assert all(max(t_mu, t_var) <= xp.ceiling(n, d) for n, d in xp.CASES)
