"""Batched acquisition engine: the device replacement for the reference's maximiser loop.

The reference maximises every acquisition with ``scipy.optimize.differential_evolution``,
calling ``acq(x)`` one candidate at a time (optimisers.py:87,118,366; emo.py:240).  Here one
BO iteration uploads the fitted surrogates once, scores a large quasi-random candidate batch
on the GPU (Sobol generation → posterior → acquisition) and reduces it with the device arg-max.  With
torch.distributed initialised, every rank scores its own contiguous shard of the Sobol
sequence and the ranks exchange one {value, index} pair (optimobo_amd.parallel); the winning
point is regenerated from its Sobol index on every rank, so no coordinates are broadcast.
"""
import numpy as np
import torch

from . import pareto
from ._lib import OMB_ENOTPD, OMBError
from .device import AcqContext
from .gp import GPState
from .paths import draw_path_inputs, feature_lengthscale
from .parallel import global_argmax, shard_range, world


def _state_of(model):
    if isinstance(model, GPState):
        return model
    if hasattr(model, "state"):
        return model.state()
    raise TypeError(f"unsupported surrogate {type(model).__name__}: expected optimobo_amd.gp.GPRegression/GPState")


class AcquisitionEngine:
    """Owns one AcqContext and the fitted GP state currently resident on the device."""

    def __init__(self, device=None):
        if device is None:
            device = torch.cuda.current_device() if torch.cuda.is_available() else 0
        self.ctx = AcqContext(device)
        self.device = self.ctx.device
        self._resident = {}
        self._stale = set()     # objectives whose device state was conditioned on top of _resident[o]
        self.condition_jitter = 0.0
        self.paths_floored = 0
        self.ystar = None           # sample_minima's last result (n_obj, S)
        self.ystar_X = None         # and its minimisers (n_obj, S, d)
        self._front_lists = None    # sample_fronts' packed box lists (coords, box_off, boxes)
        self._front_con = 0         # sample_fronts' n_con: the last models are constraints read through their paths
        self._cond_X = []           # rows ``condition`` appended to every resident state since the last upload
        self.n_obj = 0

    # ------------------------------------------------------------------ model state
    def load_models(self, models):
        for o, m in enumerate(models):
            st = _state_of(m)
            if self._resident.get(o) is not st or o in self._stale:
                self.ctx.set_gp_state(o, st)
                self._cond_X = []
                self._resident[o] = st
                self._stale.discard(o)
        self.n_obj = len(models)
        return self

    def condition(self, Xnew, Y=None):
        """Condition every loaded objective on the rows of Xnew (q, d) in place, without a refit
        (AcqContext.gp_append): ``Y`` (q, n_obj) are their values, None the Kriging believer (each point takes
        its posterior mean, so only σ² shrinks).  Returns the (q, n_obj) predictive means.  "Every loaded objective"
        includes constraint models loaded behind the objectives (``plan_constraints``): the believer conditions them
        too.

        The noise of the bordered update is the resident state's ``noise``, plus ``DeviceGPState.jitter`` when
        the device fit had to add one.  A host ``GPState`` does not record the jitter its jitchol escalated to;
        for such a state the update is exact only when the first factorisation succeeded (the usual case).

        A point the update cannot take at that noise (δ² ≤ 0: OMB_ENOTPD, the state untouched) — a proposal on
        top of a training point under a large σ_f², where the 1e-8 jitter is far below the rounding of vᵀv — is
        tried again with jitchol's escalation on the new points' diagonal, σ_n² + σ_f²·1e-6·10^t for t = 0..4
        (the appended observations are then taken as that much noisier; the points already in the state keep
        their factorisation).  ``condition_jitter`` holds the largest such addition of the last call (0.0 when
        none was needed); the OMBError is raised when even t = 4 fails.

        The touched entries are marked stale: the next ``load_models`` uploads the fitted state again even for
        the same state object, so fantasies never reach the next iteration."""
        Xnew = np.atleast_2d(np.asarray(Xnew, np.float64))
        q = Xnew.shape[0]
        if Y is not None:
            Y = np.asarray(Y, np.float64).reshape(q, self.n_obj)
        Xd = self._dev(Xnew)
        mus = np.empty((q, self.n_obj))
        self.condition_jitter = 0.0
        for o in range(self.n_obj):
            st = self._resident.get(o)
            if st is None:
                raise RuntimeError(f"condition: objective {o} holds no state (call load_models first)")
            noise = float(getattr(st, "noise", 0.0)) + float(getattr(st, "jitter", None) or 0.0)
            self._stale.add(o)
            for t in range(-1, 5):
                extra = 0.0 if t < 0 else float(st.variance) * 1e-6 * 10.0 ** t
                try:
                    mus[:, o], _ = self.ctx.gp_append(o, Xd, None if Y is None else Y[:, o], noise + extra)
                    break
                except OMBError as e:
                    if e.code != OMB_ENOTPD or t == 4:
                        raise
            self.condition_jitter = max(self.condition_jitter, extra)
        self._cond_X.append(Xnew)
        return mus

    def _dev(self, x):
        return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device=self.device)

    def posterior(self, Xc):
        Xc = Xc if isinstance(Xc, torch.Tensor) else self._dev(np.atleast_2d(Xc))
        return self.ctx.posterior(Xc, self.n_obj)

    # ------------------------------------------------------------------ acquisitions on a batch
    def ehvi(self, Xc, max_point, PF, cache, mode="reference"):
        """util_functions.EHVI (2 objectives) on every row of Xc."""
        mu, var = self.posterior(Xc)
        s00, s01 = pareto.cache_stats(np.asarray(cache, np.float64))
        pf = pareto.stripes_2d(PF)
        return self.ctx.ehvi2d(mu, var, pf, np.asarray(max_point, np.float64), s00, s01, mode=mode)

    def ehvi_2d_aux(self, PF, r, mu, sigma):
        """EHVI_2D_aux(PF, r, μ, σ) with σ given directly (util_functions.py:81), batched: (2, N)."""
        mu = self._dev(np.asarray(mu, np.float64).reshape(2, -1))
        sig = self._dev(np.asarray(sigma, np.float64).reshape(2, -1))
        return self.ctx.ehvi2d(mu, sig, pareto.stripes_2d(PF), np.asarray(r, np.float64), 1.0, 1.0, mode="sigma")

    def ehvi_exact(self, Xc, max_point, PF, max_boxes=1 << 20):
        """Exact EHVI (2 to 8 objectives) over the box decomposition — "textbook" mode.  ValueError when the
        decomposition (k ≥ 4) needs more than max_boxes boxes."""
        mu, var = self.posterior(Xc)
        coords, _, boxes = pareto.box_decomposition(PF, max_point, max_boxes=max_boxes)
        return self.ctx.ehvi_boxes(mu, var, coords, boxes)

    def hvi(self, Y, max_point, PF, max_boxes=1 << 20):
        """Hypervolume improvement HV(PF ∪ {y}) − HV(PF) of every row of Y (N, k) — host values or a device
        tensor — over the front PF (2 to 8 objectives): the box sum of omb_hvi_boxes over the decomposition
        ``ehvi_exact`` uses → device tensor (N,).  ValueError when the decomposition needs more than max_boxes."""
        coords, _, boxes = pareto.box_decomposition(PF, max_point, max_boxes=max_boxes)
        Yd = Y if isinstance(Y, torch.Tensor) else self._dev(np.atleast_2d(Y))
        return self.ctx.hvi_boxes(Yd.to(device=self.device, dtype=torch.float64).T.contiguous(), coords, boxes)

    def sample_paths(self, S, n_features=1024, seed=0, noise=None, lower=None, upper=None):
        """Install S posterior sample paths (1 ≤ S ≤ 16) on every loaded model: draws that are functions
        (pathwise conditioning on ``n_features`` random Fourier features, AcqContext.paths_set), to be evaluated
        anywhere, any number of times, with ``path_values`` until the models change.  One
        ``paths.draw_path_inputs`` + ``paths_set`` per model in model order, all draws from one
        ``numpy.random.default_rng(seed)``.  ``noise``: the σ_n² of the states' factorisation (default: each loaded
        state's own, plus the device fit's jitter where it added one).  With the box ``lower`` / ``upper`` the
        frequencies are kept inside the device cosine's argument range over it; a lengthscale below
        ``paths.feature_lengthscale``'s floor (a degenerate fit) is raised to it for the features alone, and
        ``paths_floored`` counts the (model, dimension) pairs that happened to."""
        if self.n_obj < 1:
            raise RuntimeError("sample_paths: no models loaded (call load_models first)")
        rng = np.random.default_rng(seed)
        self.paths_floored = 0      # (model, dimension) pairs whose lengthscale was below the features' floor
        self._front_lists = None    # fronts of the previous paths say nothing about these
        for o in range(self.n_obj):
            st = self._resident[o]
            info = self.ctx.gp_info[o]
            ls = np.broadcast_to(np.asarray(st.lengthscale, np.float64), (info["d"],))
            ls_f = ls if lower is None or upper is None else feature_lengthscale(ls, lower, upper)
            omega, phase, w, z = draw_path_inputs(st.kernel, info["n"], info["d"], int(S), int(n_features), rng,
                                                  lower=lower, upper=upper, lengthscale=ls_f)
            if np.any(ls_f != ls):      # the device scales x by the fitted ℓ: ω̃·(ℓ/ℓ_f)·(x/ℓ) = ω̃·(x/ℓ_f)
                omega = omega * (ls / ls_f)
                self.paths_floored += int(np.sum(ls_f != ls))
            nz = noise if noise is not None else \
                float(getattr(st, "noise", 0.0)) + float(getattr(st, "jitter", None) or 0.0)
            self.ctx.paths_set(o, omega, phase, w, z, noise=nz)
        return self

    def path_values(self, Xc):
        """The installed sample paths at Xc (N, d) → device tensor (n_obj, S, N)."""
        Xc = Xc if isinstance(Xc, torch.Tensor) else self._dev(np.atleast_2d(Xc))
        return self.ctx.paths_eval(Xc, self.n_obj)

    def nondominated(self, Y, S=1):
        """``AcqContext.nondominated`` over the engine's context: the non-dominated points of Y (k, N) — S = 1 — or
        (k, S, N), a device tensor or host values → (mask (S, N) bool, counts (S,)) on the device."""
        Yd = Y if isinstance(Y, torch.Tensor) else self._dev(Y)
        return self.ctx.nondominated(Yd.to(device=self.device, dtype=torch.float64), S)

    def _point_rows(self, Y):
        Yd = Y if isinstance(Y, torch.Tensor) else self._dev(Y)
        return Yd.to(device=self.device, dtype=torch.float64)

    def hypervolume(self, Y, ref, S=1, mask=None):
        """``AcqContext.hypervolume`` over the engine's context: the exact hypervolume below ``ref`` of Y (k, N) —
        S = 1 — or of each of the S sets of Y (k, S, N), a device tensor or host values (coordinates along the first
        axis, as ``nondominated`` takes them) → (S,) on the device."""
        return self.ctx.hypervolume(self._point_rows(Y), ref, S, mask)

    def hypervolume_contributions(self, Y, ref, mask=None):
        """``AcqContext.hypervolume_contributions`` over the engine's context: Y (k, N) → (hv (1,), contributions
        (N,)) on the device."""
        return self.ctx.hypervolume_contributions(self._point_rows(Y), ref, mask)

    def path_front_hypervolumes(self, Xc, ref):
        """The hypervolume below ``ref`` of every installed sample path's Pareto set over the candidates Xc (N, d) —
        S draws from the posterior of the attainable hypervolume → (S,) on the device.  ``path_values``,
        ``nondominated`` and ``hypervolume`` on the device tensors of one another: no value crosses to the host
        between the three calls."""
        Y = self.path_values(Xc)                                    # (n_obj, S, N)
        mask, _ = self.ctx.nondominated(Y, Y.shape[1])
        return self.ctx.hypervolume(Y, ref, Y.shape[1], mask)

    def path_fronts(self, Xc):
        """The Pareto set of every installed sample path (``sample_paths(S)``) over the candidates Xc (N, d): one
        ``path_values`` and one ``nondominated`` call over the S sets → a list of S pairs (index (P_s,) int64
        ascending, values (P_s, n_obj)) of device tensors.  What Pareto-front entropy search, joint entropy search
        and TSEMO-style batches start from."""
        Y = self.path_values(Xc)                                    # (n_obj, S, N)
        mask, _ = self.ctx.nondominated(Y, Y.shape[1])
        out = []
        for s in range(Y.shape[1]):
            idx = torch.nonzero(mask[s]).reshape(-1)
            out.append((idx, Y[:, s, :].index_select(1, idx).T.contiguous()))
        return out

    def predicted_front(self, lower, upper, n_candidates=1 << 18, seed=0, n_con=0, min_feasibility=0.5, include=None,
                        chunk=1 << 18, pof_eps=1e-5):
        """The model's Pareto set: the non-dominated set of the posterior mean of the first n_obj − ``n_con`` loaded
        models over a dense candidate set — the answer to "which designs do I keep?" when the observations are noisy
        (the observed front is made of the luckiest draws and names evaluated points only).

        Candidates: the rows of ``include`` (the training inputs, say), then the first ``n_candidates`` points of the
        device Sobol' sequence over the box seeded by ``seed``, as ``maximise`` draws them; a candidate's ``index`` is
        its place in that order.  They are taken in pieces of ``chunk``: ``posterior``; with ``n_con`` > 0 (the last
        n_con loaded models are constraint models, g ≤ 0 feasible) the candidates whose ``feasibility`` (at
        ``pof_eps``) is below ``min_feasibility`` are dropped; ``nondominated`` on the means; the survivors go to a
        pool, and one last ``nondominated`` runs over the pool.  A piece's survivors contain every point of it that
        nothing dominates, so the result does not depend on ``chunk``.  A candidate with a NaN mean is never kept.

        Returns a dict of numpy arrays in ascending candidate order — ``X`` (P, d), ``mean`` (P, k), ``var`` (P, k),
        ``index`` (P,) — and ``info``: ``chunk_survivors`` (one count per piece), ``feasible`` (candidates that passed
        the feasibility threshold; all of them without constraints), ``candidates``.  No feasible candidate gives the
        empty front with ``info["feasible"] == 0``.  The Sobol' state of the context is overwritten; plans, GP states
        and paths are left as they are."""
        lower = np.asarray(lower, np.float64).reshape(-1)
        upper = np.asarray(upper, np.float64).reshape(-1)
        d, n_con, n_cand, chunk = lower.size, int(n_con), int(n_candidates), int(chunk)
        if self.n_obj < 1:
            raise RuntimeError("predicted_front: no models loaded (call load_models first)")
        if not 0 <= n_con < self.n_obj:
            raise ValueError(f"predicted_front: n_con={n_con} outside [0, {self.n_obj - 1}] (the loaded models less "
                             "one objective)")
        if n_cand < 0 or chunk < 1:
            raise ValueError(f"predicted_front: n_candidates={n_cand} must be >= 0 and chunk={chunk} >= 1")
        k = self.n_obj - n_con
        inc = self._dev(np.empty((0, d)) if include is None else np.atleast_2d(np.asarray(include, np.float64)))
        if inc.shape[1] != d:
            raise ValueError(f"predicted_front: include has {inc.shape[1]} columns, the box {d}")
        n_inc = inc.shape[0]
        total = n_inc + n_cand
        if n_cand:
            self.ctx.set_sobol(d, lower, upper, seed=seed)
        pool_X, pool_mu, pool_var, pool_idx, survivors, feasible = [], [], [], [], [], 0
        for c0 in range(0, total, chunk):
            c1 = min(total, c0 + chunk)
            parts = []
            if c0 < n_inc:
                parts.append(inc[c0:min(c1, n_inc)])
            if c1 > n_inc:
                s0 = max(c0, n_inc) - n_inc
                parts.append(self.ctx.sobol(s0, c1 - n_inc - s0))
            X = parts[0] if len(parts) == 1 else torch.cat(parts)
            idx = torch.arange(c0, c1, dtype=torch.int64, device=self.device)
            mu, var = self.posterior(X)
            if n_con:
                keep = self.ctx.feasibility(mu[k:], var[k:], float(pof_eps)) >= float(min_feasibility)
                X, idx = X[keep], idx[keep]
                mu, var = mu[:, keep], var[:, keep]
            feasible += int(idx.numel())
            mu, var = mu[:k].contiguous(), var[:k].contiguous()
            mask, _ = self.ctx.nondominated(mu)
            m = mask[0]
            survivors.append(int(m.sum()))
            pool_X.append(X[m])
            pool_mu.append(mu[:, m])
            pool_var.append(var[:, m])
            pool_idx.append(idx[m])
        info = dict(chunk_survivors=survivors, feasible=feasible, candidates=total)
        if not pool_idx or sum(survivors) == 0:
            return dict(X=np.empty((0, d)), mean=np.empty((0, k)), var=np.empty((0, k)), index=np.empty(0, np.int64),
                        info=info)
        X, mu, var, idx = torch.cat(pool_X), torch.cat(pool_mu, 1), torch.cat(pool_var, 1), torch.cat(pool_idx)
        m = self.ctx.nondominated(mu.contiguous())[0][0]
        return dict(X=X[m].cpu().numpy(), mean=mu[:, m].T.contiguous().cpu().numpy(),
                    var=var[:, m].T.contiguous().cpu().numpy(), index=idx[m].cpu().numpy(), info=info)

    def path_values_and_grad(self, Xc):
        """The installed sample paths and their gradients at Xc (N, d) → device tensors (vals (n_obj, S, N), grad
        (n_obj, S, d, N)) (AcqContext.paths_grad); vals are bitwise ``path_values``'."""
        Xc = Xc if isinstance(Xc, torch.Tensor) else self._dev(np.atleast_2d(Xc))
        return self.ctx.paths_grad(Xc, self.n_obj)

    def sample_minima(self, S, lower, upper, n_candidates=1 << 16, seed=0, n_features=1024, refine_rounds=0, shrink=0.1,
                      n_refine=4096, polish=False):
        """The minimum of S fresh posterior sample paths of every loaded model over the box → ``ystar`` (n_obj, S) as
        numpy, kept on the engine for ``mes`` / ``plan_mes`` (max-value entropy search).

        ``sample_paths(S, n_features, seed, lower=…, upper=…)`` (1 ≤ S ≤ 16: one path install), then
        ``AcqContext.paths_min`` — the minimum is taken in the evaluation kernel, the (n_obj, S, N) matrix is never
        stored — over the first ``n_candidates`` points of the device Sobol' sequence seeded by ``seed``, and once
        more over the resident training inputs, so that each sampled minimum is at or below its path's value at every
        observed x.  With ``refine_rounds`` > 0, ``thompson_batch``'s refinement: round r evaluates ``n_refine``
        Sobol' points of the box ``shrink``^r times the bounds' size around each path's minimiser (clipped to the
        bounds; one ``paths_min`` per round, objective and path — the boxes differ) and keeps a smaller value.  With
        ``polish``, every (model, path) minimiser is then the start of a bounded L-BFGS-B run on that path's own
        gradient (Wilson et al. 2020 minimise a path by gradient descent): the n_obj·S runs advance in lockstep, each
        round is one ``path_values_and_grad`` at the active runs' points (a run reads its own path's row), and a
        smaller value is kept.  The minimisers stay on the engine as ``ystar_X`` (n_obj, S, d).  The
        installed plan and the Sobol' state of the context are overwritten; the paths stay installed."""
        S = int(S)
        if not 1 <= S <= 16:
            raise ValueError(f"sample_minima: S={S} outside [1, 16] (one path install)")
        lower = np.asarray(lower, np.float64).reshape(-1)
        upper = np.asarray(upper, np.float64).reshape(-1)
        d, k = lower.size, self.n_obj
        self.sample_paths(S, n_features=n_features, seed=seed, lower=lower, upper=upper)
        self.ctx.set_sobol(d, lower, upper, seed=seed)
        Xc = self.ctx.sobol(0, int(n_candidates))
        val, idx = self.ctx.paths_min(Xc, k)
        Xbest = Xc[idx.clamp(min=0).reshape(-1)].reshape(k, S, d)
        shared = all(np.array_equal(self._resident[o].X, self._resident[0].X) for o in range(1, k))
        for o in range(k):      # one call when the models share their inputs (the drivers' case), else one per model
            if o == 0 or not shared:
                Xt = self._dev(self._resident[o].X)
                vt, it = self.ctx.paths_min(Xt, k)
            better = vt[o] < val[o]
            val[o] = torch.where(better, vt[o], val[o])
            Xbest[o] = torch.where(better[:, None], Xt[it[o].clamp(min=0)], Xbest[o])
        ystar, Xbest = val.cpu().numpy(), Xbest.cpu().numpy()
        for rnd in range(1, int(refine_rounds) + 1):
            half = shrink ** rnd * (upper - lower) / 2
            for o in range(k):
                for s in range(S):
                    self.ctx.set_sobol(d, np.maximum(lower, Xbest[o, s] - half), np.minimum(upper, Xbest[o, s] + half),
                                       seed=seed + 104729 * rnd + o * S + s)
                    Xr = self.ctx.sobol(0, int(n_refine))
                    vr, ir = self.ctx.paths_min(Xr, k)
                    v = float(vr[o, s])
                    if v < ystar[o, s]:
                        ystar[o, s] = v
                        Xbest[o, s] = Xr[int(ir[o, s])].cpu().numpy()
        if polish:
            def own(order, X):      # run r = o·S + s reads path s of model o at its own point
                v, g = self.path_values_and_grad(X)
                v, g = v.cpu().numpy(), g.cpu().numpy()
                o, p = np.asarray(order) // S, np.asarray(order) % S
                i = np.arange(len(order))
                return v[o, p, i], g[o, p, :, i]

            X1, _ = self._lockstep_minimise(np.clip(Xbest.reshape(k * S, d), lower, upper), own, lower, upper)
            v1 = self.path_values(X1).cpu().numpy()
            for o in range(k):
                for s in range(S):
                    v = v1[o, s, o * S + s]
                    if v < ystar[o, s]:
                        ystar[o, s] = v
                        Xbest[o, s] = X1[o * S + s]
        self.ystar = ystar
        self.ystar_X = Xbest
        return ystar

    def _ystar(self, ystar, what):
        if ystar is None:
            if self.ystar is None:
                raise RuntimeError(f"{what}: no sampled minima (call sample_minima first, or pass ystar)")
            ystar = self.ystar
        return np.atleast_2d(np.asarray(ystar, np.float64))

    def mes(self, Xc, ystar=None):
        """Max-value entropy search (MESMO over several models) on every row of Xc under the sampled minima
        ``ystar`` (k, S) of the first k loaded models (None: the last ``sample_minima`` result)."""
        ystar = self._ystar(ystar, "mes")
        mu, var = self.posterior(Xc)
        k = ystar.shape[0]
        return self.ctx.mes(mu[:k], var[:k], ystar)

    def plan_mes(self, ystar=None):
        """``mes`` as the fused chain's plan (None: the last ``sample_minima`` result); ``has_gradient`` is True."""
        self.ctx.plan_mes(self._ystar(ystar, "plan_mes"))

    def sample_fronts(self, S, max_point, lower, upper, seed=0, n_features=1024, max_boxes=1 << 20, n_con=0):
        """S fresh posterior sample paths of every loaded model, evaluated at the training inputs: S draws of the latent
        objective values there and so S fronts, the integration set of the noisy EHVI (one model: S best values, the
        noisy EI's).  The paths are latent — no observation noise is added at X.

        ``sample_paths(S, n_features, seed, lower=…, upper=…)`` (1 ≤ S ≤ 16: one path install), then ``path_values``
        at the resident training inputs, which the models must share (ValueError otherwise: a front needs every
        objective at the same rows), and at the rows ``condition`` has appended since.  Per path ``pareto.calc_pf`` and ``pareto.box_decomposition(PF_s, max_point,
        max_boxes)`` (``pareto.BoxBudgetError`` propagates); with one model, ``max_point`` is None and the lists are
        ``pareto.threshold_lists`` of the paths' minima over the training inputs (``AcqContext.paths_min``).  The
        packed lists (``pareto.pack_box_lists``) are kept on the engine for ``nehvi`` / ``plan_nehvi``, which hold
        while the paths do: until a model is loaded or conditioned.  Returns the list of fronts (S arrays (P_s, k)),
        or b (S,) for one model.

        With ``n_con`` > 0 the last n_con loaded models are constraint models (g ≤ 0 feasible) and "one model" above
        reads "one objective": every path keeps the rows at which all its constraint paths are ≤ 0
        (``pareto.feasible_fronts`` on ``path_values``), so each draw has its own feasible front, and ``nehvi`` /
        ``plan_nehvi`` weight every candidate's path by its feasibility under the same draw."""
        S, n_con = int(S), int(n_con)
        if not 1 <= S <= 16:
            raise ValueError(f"sample_fronts: S={S} outside [1, 16] (one path install)")
        if self.n_obj < 1:
            raise RuntimeError("sample_fronts: no models loaded (call load_models first)")
        if not 0 <= n_con < self.n_obj:
            raise ValueError(f"sample_fronts: n_con={n_con} outside [0, {self.n_obj - 1}] (the loaded models less one "
                             "objective)")
        k = self.n_obj - n_con
        if any(not np.array_equal(self._resident[o].X, self._resident[0].X) for o in range(1, self.n_obj)):
            raise ValueError("sample_fronts: the loaded models do not share their training inputs (a front needs every "
                             "objective at the same rows)")
        if (k == 1) != (max_point is None):
            raise ValueError("sample_fronts: one model takes max_point=None (noisy EI's thresholds), several models "
                             "need the reference point")
        self._front_lists = None
        self.sample_paths(S, n_features=n_features, seed=seed, lower=lower, upper=upper)
        # the rows the device states hold: the fitted ones and, inside a believer batch, the fantasies behind them
        Xt = self._dev(np.vstack([self._resident[0].X] + self._cond_X))
        if n_con:
            F = self.path_values(Xt).cpu().numpy()                  # (k + n_con, S, n)
            out, decomps = pareto.feasible_fronts(F[:k], F[k:], max_point, max_boxes=max_boxes)
        elif k == 1:
            out = self.ctx.paths_min(Xt, 1)[0][0].cpu().numpy()
            decomps = pareto.threshold_lists(out)
        else:
            F = self.path_values(Xt).cpu().numpy()                  # (k, S, n)
            out = [pareto.calc_pf(np.ascontiguousarray(F[:, s, :].T)) for s in range(S)]
            decomps = [pareto.box_decomposition(pf, max_point, max_boxes=max_boxes) for pf in out]
        self._front_lists = pareto.pack_box_lists(decomps)
        self._front_con = n_con
        return out

    def _fronts(self, what):
        lists = self._front_lists
        if lists is None:
            raise RuntimeError(f"{what}: no sampled fronts (call sample_fronts first)")
        return lists

    def nehvi(self, Xc, eta=0.0):
        """Noisy EHVI (one model: noisy EI) on every row of Xc: the mean over the fronts of the last ``sample_fronts``
        of the hypervolume improvement of each path's value at the candidate (``path_values`` → ``hvi_paths``).
        After ``sample_fronts(n_con > 0)`` every path's improvement is weighted by the candidate's feasibility under
        the same draw (``hvi_paths_con``): the indicator at ``eta`` = 0, the sigmoid of −g/eta above."""
        lists = self._fronts("nehvi")
        k, c = lists[0].shape[1], self._front_con
        if c:
            return self.ctx.hvi_paths_con(self.path_values(Xc)[:k + c], c, *lists, eta=eta)
        if eta:
            raise ValueError("nehvi: eta smooths the constraints' indicator; the sampled fronts have no constraints")
        return self.ctx.hvi_paths(self.path_values(Xc)[:k], *lists)

    def nehvi_value_and_grad(self, X):
        """``nehvi`` and its gradient at host points X (m, d) → numpy (v (m,), g (m, d)), over the fronts of the last
        ``sample_fronts``: ``path_values_and_grad`` → ``hvi_paths_grad``.  v is bitwise ``nehvi``'s value."""
        lists = self._fronts("nehvi_value_and_grad")
        if self._front_con:
            raise ValueError("nehvi_value_and_grad: no gradient through the constraints' feasibility weight "
                             "(sample_fronts was called with n_con > 0)")
        k = lists[0].shape[1]
        y, dy = self.path_values_and_grad(X)
        v, g = self.ctx.hvi_paths_grad(y[:k], dy[:k], *lists)
        return v.cpu().numpy().astype(np.float64), g.cpu().numpy().astype(np.float64)

    def plan_nehvi(self, eta=0.0):
        """``nehvi`` as the fused chain's plan; ``has_gradient`` is False, so ``polish="auto"`` takes the stencil."""
        lists = self._fronts("plan_nehvi")
        if self._front_con:
            self.ctx.plan_hvi_paths_con(self._front_con, *lists, eta=eta)
        elif eta:
            raise ValueError("plan_nehvi: eta smooths the constraints' indicator; the sampled fronts have no constraints")
        else:
            self.ctx.plan_hvi_paths(*lists)

    def thompson_batch(self, q, lower, upper, PF=None, max_point=None, n_candidates=None, seed=0,
                       max_boxes=1 << 20, sampler="joint", n_features=1024, refine_rounds=0, shrink=0.1,
                       n_refine=4096, polish=False, n_con=0, best=None):
        """A batch of q proposals by Thompson sampling over the loaded models → (X (q, d), info).

        The candidates are the first ``n_candidates`` points of the device Sobol' sequence seeded by ``seed``
        (default TuRBO's count min(100·d, 5000); at most the 2^18 of omb_thompson_select).  Every loaded model
        gives q joint posterior draws over them (one ``posterior_samples`` call per model, z (q, N_c) per model in
        model order from ``numpy.random.default_rng(seed)``, TuRBO's jitter ladder): the surrogates are
        independent, so are their draws.  Draw b then nominates one candidate:

        * one loaded model: the candidate with the smallest drawn value (the surrogate is minimised);
        * k ≥ 2 models and a front ``PF`` with reference point ``max_point``: the candidate whose drawn
          objective vector has the largest hypervolume improvement over the front (``hvi_boxes`` once over the
          (k, q·N_c) draws, negated into ``thompson_select``).

        ``thompson_select``'s rules hold either way: the lowest index among equals, no candidate twice.  A draw
        in which no candidate improves the front has HVI ≡ 0 and so nominates the lowest-index candidate not yet
        picked — a point of the space-filling sequence: the exploration fallback.  ``info``: ``indices`` (q,),
        ``values`` (q,) the HVI (or drawn value) of each pick under its draw, ``jitter`` per model, ``zero_draws``
        the number of draws with HVI ≡ 0 (0 with one model), ``n_candidates``.  OMBError (OMB_ENOTPD) when a
        covariance cannot be factorised within the ladder; ValueError when the front needs more than max_boxes
        boxes.  The installed plan and the loaded states are left as they are.

        ``sampler="paths"`` draws functions instead (``sample_paths(q)``, q ≤ 16, ``n_features`` features per model,
        the draws of ``numpy.random.default_rng(seed)``): nothing is factorised, so OMB_ENOTPD cannot arise, and
        the candidate set defaults to 2^16 points.  Nomination is the same.  With ``refine_rounds`` > 0 every draw
        whose HVI is not ≡ 0 is then evaluated again at ``n_refine`` Sobol' points of the box ``shrink``^round times
        the bounds' size around its nominee (clipped to the bounds), and the nominee moves where its HVI under that
        draw (one model: its drawn value) strictly improves.  ``info`` gains ``sampler``, ``n_features``,
        ``refined``, the number of draws each round moved, and ``floored`` (``sample_paths``' ``paths_floored``);
        ``jitter`` is 0 per model; ``indices`` are round 0's.  With ``polish`` (``sampler="paths"`` alone) every live
        draw's nominee is then the start of a bounded L-BFGS-B run under its own draw — one model: path b is
        minimised; else draw b's HVI over the front is maximised (``hvi_paths_grad(per_path=True)`` over the front
        packed q times, entry (b, b)) — the runs advance in lockstep, the nominee moves only on strict improvement
        and never onto a point another nominee holds (runs that end in the same corner of the box), and ``info``
        gains ``polished``, the number of nominees moved.

        With ``n_con`` > 0 the last n_con loaded models are constraint models (g ≤ 0 feasible), drawn like the
        objectives (paths, or ``posterior_samples``), and "models" above reads "objectives".  Draw b nominates its best
        candidate that is feasible under the same draw, else its least violating one: the score is
        ``hvi_paths_con``'s per-path u with the violation score, over the front packed once per draw (one objective:
        the threshold ``best``, the best feasible observation), in groups of at most 16 draws, and −u goes to
        ``thompson_select``.  The refinement rounds use the same score and also move a draw with no feasible candidate
        towards less violation; ``polish`` is refused.  ``values`` are the picks' u; ``zero_draws`` counts the draws
        whose best u ≤ 0 and ``infeasible_draws`` those whose best u < 0 (no candidate feasible under the draw)."""
        lower = np.asarray(lower, np.float64).reshape(-1)
        upper = np.asarray(upper, np.float64).reshape(-1)
        n_con = int(n_con)
        if self.n_obj < 1:
            raise RuntimeError("thompson_batch: no models loaded (call load_models first)")
        if not 0 <= n_con < self.n_obj:
            raise ValueError(f"thompson_batch: n_con={n_con} outside [0, {self.n_obj - 1}] (the loaded models less one "
                             "objective)")
        if n_con and polish:
            raise ValueError("thompson_batch: polish has no gradient through the constraints' feasibility (n_con > 0)")
        d, k, q = lower.size, self.n_obj - n_con, int(q)
        if sampler not in ("joint", "paths"):
            raise ValueError(f"thompson_batch: sampler must be 'joint' or 'paths', not {sampler!r}")
        paths = sampler == "paths"
        if polish and not paths:
            raise ValueError("thompson_batch: polish needs sampler='paths' (a joint draw is no function of x)")
        if paths and q > 16:
            raise ValueError(f"thompson_batch: sampler='paths' draws at most 16 paths per call (q={q})")
        if paths:
            n_c = 1 << 16 if n_candidates is None else int(n_candidates)
        else:
            n_c = min(100 * d, 5000) if n_candidates is None else int(n_candidates)
        n_c = min(n_c, 1 << 18)
        if not 1 <= q <= n_c:
            raise ValueError(f"thompson_batch: q={q} outside [1, {n_c}] candidates")
        geo = None
        if k > 1:
            if PF is None or max_point is None:
                raise ValueError(f"thompson_batch: {k} models need the front PF and its reference point max_point")
            coords, _, boxes = pareto.box_decomposition(PF, max_point, max_boxes=max_boxes)
            if coords.shape[0] != k:
                raise ValueError(f"thompson_batch: front of {coords.shape[0]} objectives for {k} models")
            geo = (coords, boxes)
        self.ctx.set_sobol(d, lower, upper, seed=seed)
        Xc = self.ctx.sobol(0, n_c)
        if n_con and k == 1 and best is None:
            raise ValueError("thompson_batch: one objective under constraints needs best, the threshold a feasible "
                             "candidate must beat (the best feasible observation)")
        if paths:
            self.sample_paths(q, n_features=n_features, seed=seed, lower=lower, upper=upper)
            draws = self.ctx.paths_eval(Xc, k + n_con)
            jitter = [0.0] * (k + n_con)
        else:
            rng = np.random.default_rng(seed)
            draws = torch.empty((k + n_con, q, n_c), dtype=torch.float64, device=self.device)
            jitter = []
            for o in range(k + n_con):
                Z = self._dev(rng.standard_normal((q, n_c)))
                _, j = self.ctx.posterior_samples(o, Xc, Z, out=draws[o])
                jitter.append(j)
        zero = 0
        if n_con:
            one = pareto.threshold_lists([best]) if k == 1 else [(geo[0], None, geo[1])]

            def con_score(y):       # y (k + n_con, g, N), g ≤ 16 draws → their own u (g, N)
                return self.ctx.hvi_paths_con(y, n_con, *pareto.pack_box_lists(one * y.shape[1]), violation=True,
                                              per_path=True)[1]
            h = torch.cat([con_score(draws[:, b0:b0 + 16].contiguous()) for b0 in range(0, q, 16)])
            idx = self.ctx.thompson_select(-h)
            values = h[torch.arange(q, device=self.device), idx].cpu().numpy()
            top = h.max(dim=1).values.cpu().numpy()
            zero = int((top <= 0).sum())
        elif k == 1:
            score = draws[0]
            idx = self.ctx.thompson_select(score)
            values = score[torch.arange(q, device=self.device), idx].cpu().numpy()
        else:
            h = self.ctx.hvi_boxes(draws.reshape(k, q * n_c), *geo).reshape(q, n_c)
            idx = self.ctx.thompson_select(-h)
            values = h[torch.arange(q, device=self.device), idx].cpu().numpy()
            zero = int((h.max(dim=1).values <= 0).sum().item())
        idx = idx.cpu().numpy()
        X = Xc[torch.as_tensor(idx, device=self.device)].cpu().numpy()
        info = dict(indices=idx, values=values, jitter=jitter, zero_draws=zero, n_candidates=n_c)
        if n_con:
            info["infeasible_draws"] = int((top < 0).sum())
        if not paths:
            return X, info
        if n_con:
            live = top != 0         # something to gain, or some violation to lose
        else:
            live = np.ones(q, bool) if k == 1 else (h.max(dim=1).values > 0).cpu().numpy()
        refined = []
        for rnd in range(1, int(refine_rounds) + 1):
            moved = 0
            half = shrink ** rnd * (upper - lower) / 2
            for b in np.flatnonzero(live):
                self.ctx.set_sobol(d, np.maximum(lower, X[b] - half), np.minimum(upper, X[b] + half),
                                   seed=seed + 104729 * rnd + int(b))
                Xr = self.ctx.sobol(0, int(n_refine))
                vals = self.ctx.paths_eval(Xr, k + n_con)[:, b, :]
                # one model: the smallest drawn value; else the largest HVI under draw b; constraints: the largest u
                if n_con:
                    score = con_score(vals.contiguous().unsqueeze(1))[0].contiguous()
                else:
                    score = -vals[0].contiguous() if k == 1 else self.ctx.hvi_boxes(vals, *geo)
                v, i = self.ctx.argmax(score)
                v = -v if k == 1 and not n_con else v
                if i >= 0 and (v < values[b] if k == 1 and not n_con else v > values[b]):
                    X[b] = Xr[int(i)].cpu().numpy()
                    values[b] = v
                    moved += 1
            refined.append(moved)
        info.update(sampler="paths", n_features=int(n_features), refined=refined, floored=self.paths_floored)
        if polish:
            act = np.flatnonzero(live)
            lists = None if k == 1 else pareto.pack_box_lists([(geo[0], None, geo[1])] * q)

            def own(order, X):      # run r is draw act[r]: −(its score under its own draw) and the gradient of that
                b = act[np.asarray(order)]
                i = np.arange(len(order))
                y, dy = self.path_values_and_grad(X)
                if k == 1:
                    return y[0].cpu().numpy()[b, i], dy[0].cpu().numpy()[b, :, i]
                _, _, t, tg = self.ctx.hvi_paths_grad(y, dy, *lists, per_path=True)
                return -t.cpu().numpy()[b, i], -tg.cpu().numpy()[b, i, :]

            moved = 0
            if act.size:
                X1, _ = self._lockstep_minimise(np.clip(X[act], lower, upper), own, lower, upper)
                f1, _ = own(range(act.size), X1)
                for r, b in enumerate(act):
                    v = f1[r] if k == 1 else -f1[r]
                    # two runs can end in the same corner of the box: a point another nominee holds is not taken,
                    # so the batch stays free of duplicates as thompson_select left it
                    taken = any(np.array_equal(X1[r], X[o]) for o in range(q) if o != b)
                    if (v < values[b] if k == 1 else v > values[b]) and not taken:
                        X[b] = X1[r]
                        values[b] = v
                        moved += 1
            info["polished"] = moved
        return X, info

    def ehvi3d(self, Xc, max_point, PF, cache):
        """util_functions.EHVI_3D (Monte-Carlo form) on every row of Xc, for k = n_obj ≥ 3 objectives (the
        reference calls it for every n_obj != 2): (values (N,), raised (N,) int32)."""
        mu, var = self.posterior(Xc)
        hv = pareto.hypervolume(PF, max_point)
        return self.ctx.ehvi_mc(mu, var, np.asarray(cache, np.float64), np.asarray(max_point, np.float64), hv)

    def expected_decomposition(self, Xc, weights, agg_func, agg_min, cache):
        mu, var = self.posterior(Xc)
        sid, params = agg_func.device_spec()
        return self.ctx.expdec(mu, var, np.asarray(cache, np.float64), sid, params, np.asarray(weights, np.float64),
                               np.asarray(agg_func.ideal_point, np.float64), np.asarray(agg_func.max_point, np.float64),
                               float(agg_min))

    def hvpoi(self, Xc, cells):
        mu, var = self.posterior(Xc)
        return self.ctx.hvpoi(mu, var, np.ascontiguousarray(cells, dtype=np.float64))

    def ei(self, Xc, best, var_eps=0.0):
        mu, var = self.posterior(Xc)
        return self.ctx.ei(mu[0], var[0], float(best), float(var_eps))

    def pareto_ei(self, Xc, best, var_eps=1e-6):
        """KEEP's μ_pareto · EI (keep.py:142-151); models = [scalarised, pareto membership]."""
        mu, var = self.posterior(Xc)
        return self.ctx.ei_ext("pareto", mu, var, float(best), float(var_eps))

    def constrained_ei(self, Xc, best, var_eps=0.0, pof_eps=1e-5):
        """ParEGO_C2's EI · Π PoF (cparego.py:486-496); models = [aggregate, constraint_1, ...]."""
        mu, var = self.posterior(Xc)
        return self.ctx.ei_ext("constrained", mu, var, float(best), float(var_eps), float(pof_eps))

    def feasibility(self, Xc, n_con, pof_eps=1e-5):
        """Probability of feasibility Π_j Φ(−μ_j / sqrt(σ²_j + pof_eps)) on every row of Xc under the last ``n_con``
        loaded models (rows n_obj − n_con .. of the posterior), each a GP of a constraint g_j with g_j ≤ 0 feasible."""
        n_con = int(n_con)
        if not 1 <= n_con <= self.n_obj:
            raise ValueError(f"feasibility: n_con={n_con} outside [1, {self.n_obj}] loaded models")
        mu, var = self.posterior(Xc)
        return self.ctx.feasibility(mu[self.n_obj - n_con:], var[self.n_obj - n_con:], float(pof_eps))

    # log-space forms: finite, with a slope, where the values above are exactly 0.0 (AcqContext.log_ei, …)
    def log_ei(self, Xc, best, var_eps=0.0):
        mu, var = self.posterior(Xc)
        return self.ctx.log_ei(mu[:1], var[:1], float(best), float(var_eps))

    def log_constrained_ei(self, Xc, best, var_eps=0.0, pof_eps=1e-5):
        """log of ``constrained_ei``; models = [aggregate, constraint_1, ...]."""
        mu, var = self.posterior(Xc)
        return self.ctx.log_ei(mu, var, float(best), float(var_eps), float(pof_eps), kind="constrained")

    def log_ehvi_exact(self, Xc, max_point, PF, max_boxes=1 << 20):
        """log of ``ehvi_exact`` (2 to 8 objectives)."""
        mu, var = self.posterior(Xc)
        coords, _, boxes = pareto.box_decomposition(PF, max_point, max_boxes=max_boxes)
        return self.ctx.log_ehvi_boxes(mu, var, coords, boxes)

    def log_feasibility(self, Xc, n_con, pof_eps=1e-5):
        """log of ``feasibility``: finite where every candidate's probability of feasibility is 0.0."""
        n_con = int(n_con)
        if not 1 <= n_con <= self.n_obj:
            raise ValueError(f"log_feasibility: n_con={n_con} outside [1, {self.n_obj}] loaded models")
        mu, var = self.posterior(Xc)
        return self.ctx.log_feasibility(mu[self.n_obj - n_con:], var[self.n_obj - n_con:], float(pof_eps))

    # ------------------------------------------------------------------ plans (fused chain)
    # One plan per BO iteration; each candidate batch is then a single omb_eval_argmax_sobol
    # (Sobol generation → posterior → acquisition → arg-max on the device).
    def plan_ehvi(self, max_point, PF, cache, mode="reference"):
        s00, s01 = pareto.cache_stats(np.asarray(cache, np.float64))
        self.ctx.plan_ehvi2d(pareto.stripes_2d(PF), np.asarray(max_point, np.float64), s00, s01, mode=mode)

    def plan_ehvi_exact(self, max_point, PF, max_boxes=1 << 20):
        coords, _, boxes = pareto.box_decomposition(PF, max_point, max_boxes=max_boxes)
        self.ctx.plan_ehvi_boxes(coords, boxes)

    def plan_ehvi3d(self, max_point, PF, cache):
        self.ctx.plan_ehvi_mc(np.asarray(cache, np.float64), np.asarray(max_point, np.float64),
                              pareto.hypervolume(PF, max_point))

    def plan_expected_decomposition(self, weights, agg_func, agg_min, cache):
        sid, params = agg_func.device_spec()
        self.ctx.plan_expdec(np.asarray(cache, np.float64), sid, params, np.asarray(weights, np.float64),
                             np.asarray(agg_func.ideal_point, np.float64), np.asarray(agg_func.max_point, np.float64),
                             float(agg_min))

    def plan_hvpoi(self, cells):
        self.ctx.plan_hvpoi(np.ascontiguousarray(cells, dtype=np.float64))

    def plan_ei(self, best, var_eps=0.0):
        self.ctx.plan_ei(float(best), float(var_eps))

    def plan_pareto_ei(self, best, var_eps=1e-6):
        self.ctx.plan_ei_ext("pareto", 2, float(best), float(var_eps))

    def plan_constrained_ei(self, best, var_eps=0.0, pof_eps=1e-5):
        self.ctx.plan_ei_ext("constrained", self.n_obj, float(best), float(var_eps), float(pof_eps))

    def plan_constraints(self, n_con, pof_eps=1e-5):
        """Weight the plan just set by the probability of feasibility of the ``n_con`` models loaded after its
        objectives (slots k .. k + n_con − 1; g ≤ 0 feasible).  Call it after the plan_* method: every plan starts
        without constraints.  ``condition`` appends to every loaded model, so a believer batch conditions the
        constraint GPs on the fantasy points as well (their σ² shrinks there, their μ stays)."""
        self.ctx.plan_constraints(int(n_con), float(pof_eps))

    def plan_log(self, on=True):
        """The plan just set returns the logarithm of its acquisition (``plan_ei``, ``plan_constrained_ei``,
        ``plan_ehvi_exact``; OMBError OMB_EUNSUP for the others) and ``plan_constraints`` adds log F.  Before or
        after ``plan_constraints``; every plan starts linear.  ``maximise`` and the polishes work on the sign-free
        value as they are; ``has_gradient`` is False for the log exact EHVI, so ``polish="auto"`` takes the stencil."""
        self.ctx.plan_log(on)

    # ------------------------------------------------------------------ maximiser
    def score(self, acq_fn, X):
        """Acquisition values at host points X (m, d) → numpy (m,); NaN reads as −inf."""
        Xd = self._dev(np.atleast_2d(X))
        v = (self.ctx.eval(Xd) if acq_fn is None else acq_fn(Xd)).cpu().numpy().astype(np.float64)
        return np.where(np.isnan(v), -np.inf, v)

    def polish(self, acq_fn, x0, v0, lower, upper, maxiter=100):
        """Local L-BFGS-B finish from (x0, v0) — what ``differential_evolution(polish=True)`` does to its
        best member (scipy's default; optimisers.py:87,118 use it).  The objective and its central-
        difference gradient come from ONE batched device evaluation of the (2d+1)-point stencil per
        L-BFGS-B step (one-sided at the bounds).  Keeps x0 unless the polished point scores higher.
        The objective is scaled by 1/|v0|: L-BFGS-B's stopping test compares the decrease of f with
        ftol·max(|f|, 1), so an unscaled acquisition of magnitude 1e-3 would stop at a relative accuracy
        of ~1e-6 (the README run's expected decomposition is 1e-4 to 1e-2)."""
        from scipy.optimize import minimize
        lower = np.asarray(lower, np.float64)
        upper = np.asarray(upper, np.float64)
        d = lower.size
        h = 1e-6 * np.maximum(upper - lower, 1e-12)
        scale = 1.0 / abs(v0) if np.isfinite(v0) and v0 != 0.0 else 1.0

        def fg(x):
            x = np.clip(x, lower, upper)
            P = np.repeat(x[None, :], 2 * d + 1, axis=0)
            for j in range(d):
                P[1 + 2 * j, j] = min(x[j] + h[j], upper[j])
                P[2 + 2 * j, j] = max(x[j] - h[j], lower[j])
            v = self.score(acq_fn, P)
            if not np.isfinite(v[0]):
                return np.inf, np.zeros(d)
            g = np.zeros(d)
            for j in range(d):
                a, b = v[1 + 2 * j], v[2 + 2 * j]
                step = P[1 + 2 * j, j] - P[2 + 2 * j, j]
                if np.isfinite(a) and np.isfinite(b) and step > 0:
                    g[j] = (a - b) / step
            return -v[0] * scale, -g * scale

        res = minimize(fg, np.asarray(x0, np.float64), jac=True, method="L-BFGS-B",
                       bounds=list(zip(lower, upper)), options={"maxiter": int(maxiter)})
        x1 = np.clip(res.x, lower, upper)
        v1 = float(self.score(acq_fn, x1[None, :])[0])
        return (x1, v1) if v1 > v0 else (np.asarray(x0, np.float64), float(v0))

    def has_gradient(self):
        """True when the current plan is one the device differentiates (omb_eval_grad): the EI family, EHVI-2D
        in reference or textbook mode, exact EHVI over boxes."""
        return self.ctx.plan_has_gradient()

    def value_and_grad(self, X):
        """The plan's acquisition and its gradient at host points X (m, d) → numpy (v (m,), g (m, d)): one
        omb_eval_grad.  v is bitwise ``score``'s value before its NaN → −inf mapping."""
        v, g = self.ctx.eval_grad(self._dev(np.atleast_2d(X)))
        return v.cpu().numpy().astype(np.float64), g.cpu().numpy().astype(np.float64)

    def _lockstep_minimise(self, X0, own, lower, upper, maxiter=100):
        """One bounded L-BFGS-B run per row of X0 (m, d) (scipy's routine in reverse communication, gp._LbfgsbRun),
        advanced in lockstep: every round is ONE call ``own(order, X)`` → (f (len,), g (len, d)), the objectives to
        minimise of the runs ``order`` still active at their points X.  The objective of run s is f/|f(x0_s)|,
        ``polish``'s scaling; a non-finite value reads as +inf with a zero gradient, and a run whose start has one
        stays where it is.  Returns (the end points (m, d) inside the bounds, f at X0)."""
        from .gp import _LbfgsbRun, _lockstep_ok
        m, d = X0.shape
        f0, g0 = own(list(range(m)), X0)
        f0 = np.asarray(f0, np.float64)
        ok = np.isfinite(f0)
        scale = np.where(ok & (f0 != 0.0), 1.0 / np.where(ok & (f0 != 0.0), np.abs(f0), 1.0), 1.0)

        def fg(s, f, g):
            if not np.isfinite(f):
                return np.inf, np.zeros(d)
            return f * scale[s], np.where(np.isfinite(g), g, 0.0) * scale[s]

        X1 = X0.copy()
        if _lockstep_ok():
            runs = {s: _LbfgsbRun(X0[s], *fg(s, f0[s], g0[s]), 15000, int(maxiter), bounds=(lower, upper))
                    for s in range(m) if ok[s]}
            while runs:
                ask = {}
                for s in sorted(runs):
                    x = runs[s].advance()
                    if x is None:
                        X1[s] = runs.pop(s).x
                    else:
                        ask[s] = x
                if not ask:
                    break
                order = sorted(ask)
                f, g = own(order, np.stack([ask[s] for s in order]))
                for i, s in enumerate(order):
                    runs[s].supply(ask[s], *fg(s, f[i], g[i]))
        else:   # another scipy layout: the same runs one after another
            from scipy.optimize import minimize
            for s in np.flatnonzero(ok):
                def one(x, s=s):
                    f, g = own([int(s)], np.clip(x, lower, upper)[None, :])
                    return fg(s, f[0], g[0])
                X1[s] = minimize(one, X0[s], jac=True, method="L-BFGS-B", bounds=list(zip(lower, upper)),
                                 options={"maxiter": int(maxiter)}).x
        return np.clip(X1, lower, upper), f0

    def polish_batch(self, starts, lower, upper, maxiter=100, value_and_grad=None):
        """``polish`` for several starts at once on the analytic gradient: one bounded L-BFGS-B run per start
        (``_lockstep_minimise``), advanced in lockstep — every round is ONE omb_eval_grad on the points of the runs
        still active, instead of a (2d+1)-point stencil per run and step.
        ``starts``: points (m, d), or (x, v) pairs as ``_starts`` returns them (the value is taken again at x).
        The objective of run s is −a(x)/|a(x0_s)|, ``polish``'s scaling.  Returns [(x, v)] in the order of the
        starts; each keeps its x0 unless the polished point scores strictly higher.
        ``value_and_grad``: a callable X (m, d) → numpy (v (m,), g (m, d)) in place of ``self.value_and_grad`` and of
        the final ``score`` (None: the plan's own, as before)."""
        vg = self.value_and_grad if value_and_grad is None else value_and_grad
        lower = np.asarray(lower, np.float64)
        upper = np.asarray(upper, np.float64)
        d = lower.size
        if len(starts) and isinstance(starts[0], tuple):
            starts = [s[0] for s in starts]
        X0 = np.clip(np.asarray(starts, np.float64).reshape(-1, d), lower, upper)
        m = X0.shape[0]
        if m == 0:
            return []

        def own(order, X):
            v, g = vg(X)
            return -np.asarray(v, np.float64), -np.asarray(g, np.float64)

        X1, f0 = self._lockstep_minimise(X0, own, lower, upper, maxiter)
        v0 = -f0
        if value_and_grad is None:
            v1 = self.score(None, X1)
        else:
            v1 = np.asarray(value_and_grad(X1)[0], np.float64)
            v1 = np.where(np.isnan(v1), -np.inf, v1)
        v0s = np.where(np.isnan(v0), -np.inf, v0)
        return [(X1[s], float(v1[s])) if v1[s] > v0s[s] else (X0[s], float(v0s[s])) for s in range(m)]

    def _starts(self, acq_fn, lower, upper, n_candidates, seed, k, pool=64, sep=0.1):
        """Round 0 of a multi-start search: the ``n_candidates`` Sobol points scored on the device, every rank's
        ``pool`` best (value, global index) pairs gathered, then up to ``k`` starts picked greedily in
        (value desc, index asc) order — the arg-max rule, so start 0 is round 0's arg-max — each at least ``sep``
        (in units of the box) from the starts already taken.  Returns [(x, v)], best first."""
        d = lower.size
        W, rank = world()
        start, count = shard_range(n_candidates, W, rank)
        self.ctx.set_sobol(d, lower, upper, seed=seed)
        vals = self.ctx.eval(self.ctx.sobol(start, count)) if acq_fn is None else acq_fn(self.ctx.sobol(start, count))
        v = torch.nan_to_num(vals, nan=-float("inf"))
        # start 0 is round 0's arg-max by the device rule (value desc, lowest index; NaN never wins): torch.topk does
        # not promise which of several equal values it returns, so the pool alone could miss it on a flat
        # region (e.g. reference-mode EHVI <= 0 with many ties at 0)
        best = global_argmax(self.ctx.argmax_dev(vals, offset=start)).cpu().numpy()
        top = torch.topk(v, min(pool, count))
        pairs = torch.stack([top.values, top.indices.to(torch.float64) + start], 1)
        if W > 1:
            pad = torch.full((pool, 2), -float("inf"), dtype=torch.float64, device=pairs.device)
            pad[:pairs.shape[0]] = pairs
            pad[pairs.shape[0]:, 1] = -1.0
            if torch.distributed.get_backend() == "gloo":
                pad = pad.cpu()
            gathered = [torch.empty_like(pad) for _ in range(W)]
            torch.distributed.all_gather(gathered, pad)
            pairs = torch.cat(gathered)
        P = pairs.cpu().numpy()
        P = P[(P[:, 1] >= 0) & np.isfinite(P[:, 0])]
        P = P[np.lexsort((P[:, 1], -P[:, 0]))]
        if best[1] >= 0 and np.isfinite(best[0]):
            P = np.concatenate([best[None, :], P[P[:, 1] != best[1]]])
        span = np.maximum(upper - lower, 1e-300)
        out = []
        for val, idx in P:
            x = self.ctx.sobol(int(idx), 1).cpu().numpy()[0]
            if all(np.max(np.abs(x - y) / span) >= sep for y, _ in out):
                out.append((x, float(val)))
            if len(out) == k:
                break
        return out

    def maximise(self, acq_fn, lower, upper, n_candidates=1 << 16, seed=0, refine_rounds=2, shrink=0.1,
                 polish=True, starts=None):
        """Arg-max of the acquisition over [lower, upper]^d.

        ``acq_fn`` is None for the current plan (fused chain, one C call per batch) or a callable
        ``acq_fn(Xc_tensor (N, d)) -> (N,) tensor``.  Round 0 scores the first ``n_candidates``
        points of a scrambled Sobol sequence generated on the device (seeded, so every rank sees
        the same sequence and owns one contiguous shard).  Each refinement round re-centres a box
        ``shrink`` times smaller on the incumbent and keeps it if it improves.  ``polish`` then
        finishes with L-BFGS-B from the incumbent, as scipy's differential_evolution does by
        default (``polish``); with several ranks rank 0 polishes and broadcasts the point.
        ``starts`` (default: 1 for n_var ≤ 2, 4 above): independent incumbents refined and polished from
        round 0's best well-separated points (_starts) — round 0's arg-max alone stopped 1.2% short of
        scipy's DE on a 6-D expected decomposition (tests/test_gpu_config1.py); the first start is the
        single-start search's, so the result is never worse.
        ``polish="analytic"`` finishes all starts together, after their refinement rounds, with ``polish_batch``
        (L-BFGS-B on the device gradient, one omb_eval_grad per round for all starts); it needs the plan
        (``acq_fn`` None) and a plan with a gradient (``has_gradient``), ValueError otherwise.  ``polish="auto"``
        is "analytic" where that applies and the stencil polish (True) elsewhere.
        ``polish="paths"`` is the same finish under the noisy EHVI / noisy EI plan, whose gradient goes through the
        sample paths (``nehvi_value_and_grad``: omb_paths_grad → omb_hvi_paths_grad, one pair per round for all
        starts); it needs ``acq_fn`` None, the plan set by ``plan_nehvi`` and its fronts still on the engine,
        ValueError otherwise.
        Returns (x_best (d,), value).
        """
        lower = np.asarray(lower, np.float64)
        upper = np.asarray(upper, np.float64)
        d = lower.size
        W, rank = world()
        if polish == "paths":
            kind = self.ctx.plan_kind
            if acq_fn is not None or kind is None or kind[0] != "omb_plan_hvi_paths" or self._front_lists is None:
                raise ValueError("polish='paths' needs the planned acquisition (acq_fn=None), the plan set by "
                                 "plan_nehvi and the fronts of sample_fronts still on the engine")
        elif isinstance(polish, str):
            if polish not in ("analytic", "auto"):
                raise ValueError(f"polish must be True, False, 'analytic', 'auto' or 'paths', not {polish!r}")
            can = acq_fn is None and self.has_gradient()
            if polish == "analytic" and not can:
                raise ValueError("polish='analytic' needs the planned acquisition (acq_fn=None) and a plan with a "
                                 "device gradient (EI family, EHVI-2D reference / textbook, exact EHVI over boxes)")
            polish = "analytic" if can else True
        k = (1 if d <= 2 else 4) if starts is None else int(starts)
        if k > 1:
            cands = self._starts(acq_fn, lower, upper, n_candidates, seed, k)
        else:
            start, count = shard_range(n_candidates, W, rank)
            self.ctx.set_sobol(d, lower, upper, seed=seed)
            if acq_fn is None:
                pair = self.ctx.eval_argmax_sobol(start, count)
            else:
                pair = self.ctx.argmax_dev(acq_fn(self.ctx.sobol(start, count)), offset=start)
            g = global_argmax(pair).cpu().numpy()
            cands = [(self.ctx.sobol(int(g[1]), 1).cpu().numpy()[0], float(g[0]))] if g[1] >= 0 else []
        if not cands:   # every candidate was NaN/−inf: fall back to the first Sobol point
            self.ctx.set_sobol(d, lower, upper, seed=seed)
            return self.ctx.sobol(0, 1).cpu().numpy()[0], -np.inf
        results = []
        for best_x, best_v in cands:
            for rnd in range(1, refine_rounds + 1):
                half = shrink ** rnd * (upper - lower) / 2
                lo = np.maximum(lower, best_x - half)
                hi = np.minimum(upper, best_x + half)
                start, count = shard_range(n_candidates, W, rank)
                self.ctx.set_sobol(d, lo, hi, seed=seed + rnd)
                if acq_fn is None:
                    pair = self.ctx.eval_argmax_sobol(start, count)
                else:
                    pair = self.ctx.argmax_dev(acq_fn(self.ctx.sobol(start, count)), offset=start)
                g = global_argmax(pair).cpu().numpy()
                if g[1] >= 0 and g[0] > best_v:
                    best_x = self.ctx.sobol(int(g[1]), 1).cpu().numpy()[0]   # the winner, regenerated
                    best_v = float(g[0])
            if polish and polish not in ("analytic", "paths"):
                if W == 1:
                    best_x, best_v = self.polish(acq_fn, best_x, best_v, lower, upper)
                else:
                    box = [None]
                    if rank == 0:
                        box[0] = self.polish(acq_fn, best_x, best_v, lower, upper)
                    torch.distributed.broadcast_object_list(box, src=0)
                    best_x, best_v = np.asarray(box[0][0], np.float64), float(box[0][1])
            results.append((best_x, best_v))
        if polish in ("analytic", "paths"):
            vg = self.nehvi_value_and_grad if polish == "paths" else None
            if W == 1:
                results = self.polish_batch(results, lower, upper, value_and_grad=vg)
            else:
                box = [None]
                if rank == 0:
                    box[0] = self.polish_batch(results, lower, upper, value_and_grad=vg)
                torch.distributed.broadcast_object_list(box, src=0)
                results = [(np.asarray(x, np.float64), float(v)) for x, v in box[0]]
        # the best start; ties to the earliest (the single-start search's when it ties)
        return max(results, key=lambda r: r[1])


_ENGINES = {}


def device_engine(device=None):
    """The process-wide engine of ``device``, whatever models it holds (for what reads none: ``hypervolume``)."""
    if device is None:
        device = torch.cuda.current_device() if torch.cuda.is_available() else 0
    eng = _ENGINES.get(device)
    if eng is None:
        eng = _ENGINES[device] = AcquisitionEngine(device)
    return eng


def engine_for(models, device=None):
    """Process-wide engine per device with ``models`` resident."""
    return device_engine(device).load_models(models)
