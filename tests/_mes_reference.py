"""References for max-value entropy search (omb_mes, omb_plan_mes).

  * mpmath references at 60 digits: a(γ) = γφ(γ)/(2Φ(γ)) − log Φ(γ) and α = Σ_j (Σ_s a(γ_js))/S, with Φ from erfc so
    that it does not underflow;
  * an fp64 numpy restatement of the device forms (omb_math.h's mes_term on tail_ratios, omb_mes.hip's kernels);
  * the inputs that tests/test_mes_host.py (CPU) and tests/test_gpu_mes.py (GPU) share: γ walks _logacq_reference's
    GAMMAS at every σ² of VARS, for (k, S) = (1, 1), (3, 5) and (8, 64).

Everything here is computed once per process (functools.lru_cache) and must be left unchanged by its users.
"""
import functools

import mpmath as mp
import numpy as np
from scipy.special import erfc, ndtr

from _logacq_reference import GAMMAS, VARS, _mpf, err, tail_ratios  # noqa: F401  (err: re-exported to the tests)

LOG_SQRT_2PI = 0.91893853320467274178
SQRT1_2 = 0.70710678118654752440
CASES = ((1, 1), (3, 5), (8, 64))        # (k, S)
N_ACC = 1000                             # candidates of the accuracy inputs


# ----------------------------------------------------------------------------------------------- mpmath
def mp_a(g):
    """a(γ) at 60 digits; Φ = erfc(−γ/√2)/2 keeps its relative accuracy in the lower tail."""
    g = _mpf(g)
    Phi = mp.erfc(-g / mp.sqrt(2)) / 2
    return g * mp.npdf(g) / (2 * Phi) - mp.log(Phi)


@functools.lru_cache(maxsize=None)
def _mp_term(m, v, y):
    return mp_a((mp.mpf(m) - mp.mpf(y)) / mp.sqrt(mp.mpf(v)))


def mp_mes(mu, var, ystar):
    """α of one candidate: mu, var (k,), ystar (k, S); mu / var may hold mpf entries (finite-difference points).  The
    terms of fp64 inputs are cached: the shared inputs repeat their (μ, σ², y*) triples across rows."""
    tot = mp.mpf(0)
    for j in range(len(mu)):
        if isinstance(mu[j], mp.mpf) or isinstance(var[j], mp.mpf):
            sd = mp.sqrt(_mpf(var[j]))
            terms = [mp_a((_mpf(mu[j]) - _mpf(y)) / sd) for y in ystar[j]]
        else:
            terms = [_mp_term(float(mu[j]), float(var[j]), float(y)) for y in ystar[j]]
        tot += sum(terms) / len(ystar[j])
    return tot


# ----------------------------------------------------------------------------------------------- fp64 restatement
def _npdf(t):
    return np.exp(-(t * t) / 2.0) / 2.5066282746310002


def _terms(g):
    """(a, a') of mes_term: the tail-ratio forms below 0 (D by its series below −30), the direct ones from 0 up."""
    g = np.asarray(g, np.float64)
    with np.errstate(all="ignore"):
        gn = np.minimum(g, -0.0)
        R, T = tail_ratios(gn)
        a_lo = (gn * T / (2.0 * R) + LOG_SQRT_2PI) - np.log(R)
        w = 1.0 / (gn * gn)
        n = 2.0 * w * (1.0 - w * (6.0 - w * (45.0 - w * (420.0 - w * (4725.0 - w * (62370.0 - w * 945945.0))))))
        D = np.where(gn > -30.0, 1.0 + gn * T / R, n / (1.0 - T))
        da_lo = -D / (2.0 * R)
        q = _npdf(g) / ndtr(g)
        a_hi = g * q / 2.0 - np.log1p(-(0.5 * erfc(g * SQRT1_2)))
        da_hi = -(q / 2.0) * ((1.0 + g * g) + g * q)
    lo = g < 0.0
    return np.where(lo, a_lo, a_hi), np.where(lo, da_lo, da_hi)


def a(g):
    return _terms(g)[0]


def a_prime(g):
    return _terms(g)[1]


def naive_a(g):
    """γφ/(2Φ) − log Φ as written: what the device forms replace (−inf at −38, NaN from −39 down)."""
    g = np.asarray(g, np.float64)
    with np.errstate(all="ignore"):
        return g * _npdf(g) / (2.0 * ndtr(g)) - np.log(ndtr(g))


def _gammas(mu, var, ystar):
    mu, var = np.atleast_2d(mu), np.atleast_2d(var)
    ystar = np.atleast_2d(np.asarray(ystar, np.float64))
    with np.errstate(all="ignore"):
        sd = np.where(var > 0.0, np.sqrt(var), np.nan)
        return sd, (mu[:, None, :] - ystar[:, :, None]) / sd[:, None, :]        # (k, S, N)


def mes(mu, var, ystar):
    """mes_kernel over rows (k, N) and ystar (k, S): Σ_j (Σ_s a(γ_js))/S, both sums in index order."""
    _, g = _gammas(mu, var, ystar)
    k, S, N = g.shape
    A = a(g)
    out = np.zeros(N)
    for j in range(k):
        sj = np.zeros(N)
        for s in range(S):
            sj = sj + A[j, s]
        out = out + sj / S
    return out


def mes_partials(mu, var, ystar):
    """∂α/∂μ_j, ∂α/∂σ²_j (k, N) (mes_grad_kernel)."""
    sd, g = _gammas(mu, var, ystar)
    k, S, N = g.shape
    dA = a_prime(g)
    dm, dv = np.zeros((k, N)), np.zeros((k, N))
    with np.errstate(all="ignore"):
        for j in range(k):
            sm, sv = np.zeros(N), np.zeros(N)
            for s in range(S):
                sm = sm + dA[j, s]
                sv = sv + dA[j, s] * (-g[j, s])
            dm[j] = (sm / S) / sd[j]
            dv[j] = (sv / S) / (2.0 * (sd[j] * sd[j]))
    return dm, dv


# ----------------------------------------------------------------------------------------------- shared inputs
@functools.lru_cache(maxsize=None)
def inputs(k, S):
    """(mu (k, N), var (k, N), ystar (k, S)), N = N_ACC.

    Base pairs (γ, σ²): the cross product GAMMAS × VARS, shuffled; column i takes pair i mod P with
    P = min(N, 8192 // S), so that the 60-digit reference evaluates at most 8192 distinct terms per case (a term
    costs 0.4 ms; (1, 1) and (3, 5) walk 1000 distinct pairs, (8, 64) 128 of them over its 1000 columns).  The sampled
    minima of row 0 are Y_s = 0.3 + s·0.01/(S − 1) and μ = Y_0 + γσ, so sample 0 meets the grid's γ and sample s sits
    at γ − s·δ/σ: on the grid's ranges again where σ is near δ, far into the lower tail (to −1e10) where σ is small.
    Row j holds the same pairs rolled by 41j columns and the same minima rolled by 5j samples: every row sums other
    terms in another order, from a set of triples the reference has already evaluated."""
    g, v = np.meshgrid(GAMMAS, VARS, indexing="ij")
    g, v = g.ravel(), v.ravel()
    perm = np.random.default_rng(23).permutation(g.size)
    col = np.arange(N_ACC) % min(N_ACC, 8192 // S)
    g, v = g[perm][col], v[perm][col]
    Y = 0.3 + np.arange(S) * (0.01 / max(1, S - 1))
    m0 = Y[0] + g * np.sqrt(v)
    mu = np.stack([np.roll(m0, 41 * j) for j in range(k)])
    var = np.stack([np.roll(v, 41 * j) for j in range(k)])
    ys = np.stack([np.roll(Y, 5 * j) for j in range(k)])
    for arr in (mu, var, ys):
        arr.setflags(write=False)
    return mu, var, ys


@functools.lru_cache(maxsize=None)
def reference(k, S):
    """mpmath α of inputs(k, S) as float64 (N,)."""
    mu, var, ys = inputs(k, S)
    return np.array([float(mp_mes(mu[:, i], var[:, i], ys)) for i in range(mu.shape[1])])


@functools.lru_cache(maxsize=None)
def grid_gammas():
    """GAMMAS as the term-level checks use them (read-only)."""
    g = np.array(GAMMAS, np.float64)
    g.setflags(write=False)
    return g
