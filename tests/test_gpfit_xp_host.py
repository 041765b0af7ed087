"""CPU: the extended-precision reference of the GP fit (tests/_gpfit_xp.py), held honest without a GPU.

  a. The reference checks itself: every gradient entry is the central difference of its own log p(y) in 50-digit
     arithmetic, and 80 digits give what 50 give.
  b. optimobo_amd.gp's numpy path — the specification of the device fit — is held to the reference on
     every case, noise fixed and noise free, within 4 × what ``host_fit`` (the same arithmetic) achieves in the same
     regime.  This pins the parametrisation and the signs the device is compared through.
  c. The yardstick table: ``host_fit``'s e on every case, and the conditions the helper asserts on its own inputs
     (no jitter retry is legitimate; the optimum regime is the cancelling one).
"""
import mpmath as mp
import numpy as np
import pytest

import _gpfit_xp as gx

TABLE = gx.table()


# ----------------------------------------------------------------------------- a. the reference against itself
@pytest.mark.parametrize("regime", ["late", "noisy"])
@pytest.mark.parametrize("kernel", ["matern52", "rbf"])
def test_reference_gradient_is_its_central_difference(kernel, regime):
    n, d, h = 17, 3, mp.mpf("1e-18")
    ref = gx.reference(n, d, kernel, regime)
    entries = list(ref.grad) + ([ref.grad_noise] if regime == "noisy" else [])      # σ_n² = 0 has no log
    with mp.workdps(50):
        for q, g in enumerate(entries):
            up, down = ([mp.mpf(0)] * (d + 2) for _ in range(2))
            up[q], down[q] = h, -h
            fd = (gx.lml_at(n, d, kernel, regime, tuple(up)) - gx.lml_at(n, d, kernel, regime, tuple(down))) / (2 * h)
            rel = abs(fd - g) / abs(g)
            print(f"{kernel} {regime} entry {q}: g {float(g):+.6e}  |fd - g| / |g| {float(rel):.1e}")
            assert rel <= mp.mpf("1e-25"), (q, float(rel))


def test_reference_at_80_digits():
    c = (17, 3, "matern52", "optimum")
    r50, r80 = gx.reference(*c), gx.reference(*c, dps=80)
    with mp.workdps(80):
        rels = [abs(a - b) / abs(b) for a, b in zip([r50.lml] + list(r50.grad), [r80.lml] + list(r80.grad))]
    print(f"{gx.case_id(c)}: |dps 50 - dps 80| / |dps 80|: lml {float(rels[0]):.1e}  grad {[f'{float(v):.1e}' for v in rels[1:]]}")
    assert max(rels) <= mp.mpf("1e-35")


# ----------------------------------------------------------------------------- b. the numpy path of optimobo_amd.gp
def _model(c, free):
    from optimobo_amd.gp import RBF, GPRegression, Matern52
    n, d, kernel, regime = c
    X, y, ls, sf2, noise = gx.inputs(*c)
    kern = (Matern52 if kernel == "matern52" else RBF)(d, variance=sf2, lengthscale=np.array(ls), ARD=True)
    m = GPRegression(X, y[:, None], kern, device_fit=False)
    if free:
        m.Gaussian_noise.variance.values[:] = noise
        m.Gaussian_noise.variance.unfix()
    else:
        m.Gaussian_noise.variance.fix(noise)
    return m


# σ_n² = 0 has no log: the free-noise parametrisation exists in the noisy regime only
@pytest.mark.parametrize("c,free", [(c, False) for c in TABLE] + [(c, True) for c in TABLE if c[3] == "noisy"],
                         ids=lambda v: gx.case_id(v) if isinstance(v, tuple) else ("noise-free" if v else "noise-fixed"))
def test_numpy_path_of_gp(c, free):
    n, d, kernel, regime = c
    X, y, ls, sf2, noise = gx.inputs(*c)
    m = _model(c, free)
    f, g = m._neg_lml_and_grad(m._get_free())
    # the log parametrisation handed the reference's own bits on
    assert float(m.kern.variance) == sf2 and np.array_equal(m.kern.ls_vector(), ls)
    assert float(m.Gaussian_noise.variance) == noise
    assert g.shape == (d + 2 if free else d + 1,)
    ref, bars = gx.reference(*c), gx.bars()
    e, _ = gx.errors(ref, -f, -g[:d + 1], -g[d + 1] if free else None)
    yard = gx.host_error(*c)
    t = dict(bars[regime], lml=bars["lml"])
    print(f"{gx.case_id(c)} {'free' if free else 'fixed'}: " +
          "  ".join(f"e_{k} {e[k]:.3g} (host_fit {yard[k]:.3g}, T {t[k]:.3g})" for k in e))
    for k in e:
        assert e[k] <= t[k], (k, e[k], t[k])


# ----------------------------------------------------------------------------- c. the yardstick and the inputs
def test_yardstick_table_and_input_conditions():
    for c in TABLE:
        ref = gx.reference(*c)          # asserts: smallest pivot ≥ 0.99·base, no accidental retry, |g| ≪ S at the optimum
        e = gx.host_error(*c)
        print(f"{gx.case_id(c)}: cond {ref.cond:.1e}  smallest pivot {ref.min_pivot:.3g}  S_lml {ref.s_lml:.2g}  "
              f"max|g| / max S {max(abs(float(v)) for v in ref.grad) / ref.s_grad.max():.1e}   host_fit e: " +
              "  ".join(f"{k} {v:.3g}" for k, v in e.items()))
        assert all(np.isfinite(v) for v in e.values())
    bars = gx.bars()
    print(f"bars (4 x worst host_fit e): lml {bars['lml']:.3g}; " +
          "; ".join(f"{r}: " + " ".join(f"{k} {v:.3g}" for k, v in bars[r].items()) for r in gx.REGIMES))
    # every route keeps a case in the cancelling regime
    kept = {(n, d) for n, d, _, regime in TABLE if regime == "optimum"}
    assert kept == set(gx.OPTIMUM_CASES)


def test_regimes_are_what_they_claim():
    """late and optimum are as ill-conditioned as the jitter allows, noisy is well-conditioned; the hyperparameters
    are within an ulp of late_run_state's."""
    import _posterior_xp as pxp
    for n, d in gx.CASES:
        st = pxp.late_run_state(n, d, "matern52")
        X, ys, ls, sf2 = gx.data(n, d)
        assert np.array_equal(X, st.X) and np.array_equal(ys[0], st.y[:, 0])
        assert np.all(np.abs(ls - st.lengthscale) <= 2 * np.spacing(st.lengthscale))
        assert abs(sf2 - st.variance) <= 2 * np.spacing(st.variance)
    for c in TABLE:
        cond = gx.reference(*c).cond
        if c[0] >= 15:
            assert (cond <= 1e8) if c[3] == "noisy" else (cond >= 1e8), (c, cond)
