"""CPU: the extended-precision gradient reference of tests/_grad_xp.py, held honest without a GPU.

  a. ``reference_grad`` (np.longdouble) against an independent 50-digit mpmath evaluation of the same contract, all 44
     candidates, within 2⁻⁶⁰·S entry-wise: the 64-bit significand's own error over sums of at most n ≤ 50 < 2⁷ terms;
  b. the fp64 restatement's normalised error is finite over the whole table (printed per group); a zero scale can
     occur only in the RBF far and ray entries, where every term is exactly 0 and so is the restatement.  This is what
     makes the run-time bar of tests/test_gpu_grad_xp.py well defined;
  c. fourth-order central differences of the longdouble posterior reference agree with the analytic longdouble
     gradient to 1e-6 of the term sum on the ``uniform`` group: the formulas themselves, at jitter-only conditioning.
     Near the cluster a difference quotient measures rounding (tests/test_grad_reference.py says why), so only that
     group is used.
"""
import numpy as np
import pytest

import _grad_xp as gx
import _posterior_xp as xp
import test_grad_reference as ref

LD = np.longdouble
ALL = [(n, d, k) for n, d in xp.CASES for k in xp.KERNELS]


# ----------------------------------------------------------------------------- a. helper against mpmath
def _mp_gradients(st, Xc, kernel):
    import mpmath as mp
    mp.mp.dps = 50
    f = lambda a: [mp.mpf(float(v)) for v in a]  # noqa: E731
    X = [f(row) for row in st.X]
    ls, alpha, sf2 = f(st.lengthscale), f(np.asarray(st.alpha).reshape(-1)), mp.mpf(float(st.variance))
    Linv = [f(row) for row in st.Linv]
    n, d, s5 = len(X), len(ls), mp.sqrt(5)
    dmu, dvar = [], []
    for xrow in Xc:
        x = f(xrow)
        k, g = [], []
        for i in range(n):
            r2 = mp.fsum(((x[j] - X[i][j]) / ls[j]) ** 2 for j in range(d))
            if kernel == "matern52":
                r = mp.sqrt(r2)
                k.append(sf2 * (1 + s5 * r + mp.mpf(5) / 3 * r2) * mp.exp(-s5 * r))
                g.append(-(mp.mpf(5) / 3) * sf2 * (1 + s5 * r) * mp.exp(-s5 * r))
            else:
                k.append(sf2 * mp.exp(-r2 / 2))
                g.append(-k[-1])
        v = [mp.fsum(Linv[i][c] * k[c] for c in range(i + 1)) for i in range(n)]
        w = [mp.fsum(Linv[c][i] * v[c] for c in range(i, n)) for i in range(n)]
        dmu.append([mp.fsum(alpha[i] * g[i] * (x[j] - X[i][j]) / ls[j] ** 2 for i in range(n)) for j in range(d)])
        dvar.append([-2 * mp.fsum(w[i] * g[i] * (x[j] - X[i][j]) / ls[j] ** 2 for i in range(n)) for j in range(d)])
    return dmu, dvar


@pytest.mark.parametrize("kernel", xp.KERNELS)
@pytest.mark.parametrize("n,d", [(20, 2), (50, 4)])
def test_reference_matches_mpmath(n, d, kernel):
    import mpmath as mp
    st, Xc, _, rg, (s_mu, s_var) = gx.case(n, d, kernel)
    dmu, dvar = _mp_gradients(st, Xc, kernel)
    # a longdouble converts to mpmath exactly as the sum of its fp64 head and tail
    ld = lambda z: mp.mpf(float(z)) + mp.mpf(float(z - LD(float(z))))  # noqa: E731
    worst_mu = worst_var = 0.0
    for c in range(xp.N_CAND):
        for j in range(d):
            assert s_mu[c, j] > 0
            worst_mu = max(worst_mu, float(abs(ld(rg.dmu[c, j]) - dmu[c][j]) / ld(s_mu[c, j])))
            if s_var[c, j] == 0:      # RBF far away: K* underflows even the longdouble's range (below 1e-4900)
                assert kernel == "rbf" and c >= gx.N_NEAR and rg.dvar[c, j] == 0
                assert abs(dvar[c][j]) < mp.mpf(10) ** -4900
                continue
            worst_var = max(worst_var, float(abs(ld(rg.dvar[c, j]) - dvar[c][j]) / ld(s_var[c, j])))
    print(f"n={n} d={d} {kernel}: |longdouble - mpmath| / S: dmu 2^{np.log2(max(worst_mu, 1e-300)):.1f} "
          f"dvar 2^{np.log2(max(worst_var, 1e-300)):.1f}")
    assert worst_mu <= 2.0 ** -60 and worst_var <= 2.0 ** -60


# ----------------------------------------------------------------------------- b. the yardstick is well defined
def test_restatement_error_is_finite_and_zero_only_where_every_term_is():
    for n, d, kernel in ALL:
        st, Xc, _, rg, (s_mu, s_var) = gx.case(n, d, kernel)
        dm, dv = gx.restatement_grad(st, Xc, kernel)
        assert np.all(np.isfinite(dm)) and np.all(np.isfinite(dv))
        zero = np.asarray((s_mu == 0) | (s_var == 0))
        if zero.any():                                    # only where the kernel underflowed
            assert kernel == "rbf" and not zero[:gx.N_NEAR].any()
        if kernel == "rbf":       # far and ray: every term is below fp64's smallest number, so exactly 0 in fp64
            assert np.all(rg.am[gx.N_NEAR:] < LD(1e-320)) and np.all(rg.avk[gx.N_NEAR:] < LD(1e-320))
            assert np.all(dm[gx.N_NEAR:] == 0.0) and np.all(dv[gx.N_NEAR:] == 0.0)
        e = gx.restatement_error(n, d, kernel)
        assert all(np.isfinite(v) for pair in e.values() for v in pair), e
        print(f"n={n} d={d} {kernel}: restatement e (dmu / dvar): "
              + "  ".join(f"{g} {e[g][0]:.3g}/{e[g][1]:.3g}" for g, _, _ in xp.GROUPS))
    T = gx.bar()
    print("bar T = 4 x worst per group (dmu / dvar): " + "  ".join(f"{g} {T[g][0]:.3g}/{T[g][1]:.3g}" for g in T))
    assert set(T) == {g for g, _, _ in gx.NEAR}
    for n, d in xp.CASES:
        assert all(0 < t <= gx.ceiling(n, d) for pair in T.values() for t in pair)


def test_true_gradient_spans_many_orders_of_the_scale():
    """Why the bar is relative and per group: |∂σ²/∂x| itself is anywhere from far below to far above one rounding
    of S near the data, so a bound of a few u·S alone would pass a wrong gradient."""
    lo, hi = np.inf, 0.0
    for n, d, kernel in ALL:
        _, _, _, rg, (_, s_var) = gx.case(n, d, kernel)
        q = np.asarray(np.abs(rg.dvar[:gx.N_NEAR]) / (LD(xp.U) * s_var[:gx.N_NEAR]), np.float64)
        lo, hi = min(lo, float(q[q > 0].min())), max(hi, float(q.max()))
    print(f"|dvar| / (u S) over the near groups of the table: {lo:.2e} .. {hi:.2e}")
    assert lo <= 1.0 and hi >= 1e3


# ----------------------------------------------------------------------------- c. the formulas, by differences
H_FD = 1e-3    # truncation (∝ h⁴, lengthscales ≥ 0.7) and the longdouble reference's rounding (∝ 2⁻⁶⁴·cond/h) are
               # both far below 1e-6 of the term sum


@pytest.mark.parametrize("kernel", xp.KERNELS)
@pytest.mark.parametrize("n,d", [(50, 4), (130, 6)])
def test_reference_gradient_vs_richardson(n, d, kernel):
    st, Xc, _, rg, _ = gx.case(n, d, kernel)
    lo, hi = next((a, b) for name, a, b in xp.GROUPS if name == "uniform")
    Xu = np.array(Xc[lo:hi])

    # the stencil's differences are taken in longdouble (the reference returns it); only the quotient is stored in fp64
    fm = ref.richardson(lambda X: xp.reference(st, X, kernel)[0], Xu, H_FD)
    fv = ref.richardson(lambda X: xp.reference(st, X, kernel)[1], Xu, H_FD)
    em = float(np.max(np.abs(rg.dmu[lo:hi] - fm) / rg.am[lo:hi]))
    ev = float(np.max(np.abs(rg.dvar[lo:hi] - fv) / rg.av[lo:hi]))
    print(f"n={n} d={d} {kernel}: worst |analytic - FD| / sum|terms| on the uniform group: dmu {em:.2e} dvar {ev:.2e}")
    assert em <= 1e-6 and ev <= 1e-6
