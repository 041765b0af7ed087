"""Device context: torch tensors as device-memory holders around the HIP C-ABI.

``AcqContext`` owns one ``omb_ctx`` (one per GPU) and runs every call on torch's current
stream, so torch events time the kernels exactly.  All arrays are fp64 CUDA (HIP) tensors;
the context never copies candidates to the host.
"""
import ctypes

import numpy as np
import torch

from . import _lib


_KERNEL_IDS = {"matern52": _lib.KERNEL_MATERN52, "rbf": _lib.KERNEL_RBF}
_EHVI_MODES = {"reference": _lib.EHVI_REFERENCE, "textbook": _lib.EHVI_TEXTBOOK, "sigma": _lib.EHVI_SIGMA}
_EI_KINDS = {"plain": _lib.EI_PLAIN, "pareto": _lib.EI_PARETO, "constrained": _lib.EI_CONSTRAINED}


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _dev_f64(x, device):
    if isinstance(x, torch.Tensor):
        t = x.to(device=device, dtype=torch.float64)
    else:
        t = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device=device)
    return t.contiguous()


class AcqContext:
    """One HIP context on ``device`` holding the fitted GPs of up to 8 objectives."""

    def __init__(self, device=0):
        if not torch.cuda.is_available():
            raise RuntimeError("AcqContext needs a ROCm GPU (torch.cuda.is_available() is False); "
                               "the acquisition hot path has no CPU fallback")
        self.lib = _lib.load()
        self.device = torch.device("cuda", device if isinstance(device, int) else torch.device(device).index or 0)
        h = ctypes.c_void_p()
        rc = self.lib.omb_create(self.device.index, ctypes.byref(h))
        if rc != 0:
            raise _lib.OMBError(rc, f"omb_create(device={self.device.index}) failed")
        self._h = h
        self._gp_keep = {}     # device tensors referenced by the packed GP state
        self.gp_info = {}
        self.plan_kind = None  # (omb_plan_* name, mode) of the plan last set through this object
        self.plan_is_log = False   # plan_log's flag on that plan
        self._paths_S = {}     # objective → S of the sample paths last installed through this object

    # ------------------------------------------------------------------ plumbing
    def _check(self, rc, what):
        if rc != 0:
            msg = self.lib.omb_last_error(self._h)
            raise _lib.OMBError(rc, f"{what}: {msg.decode() if msg else ''}")

    def _stream(self):
        s = torch.cuda.current_stream(self.device).cuda_stream
        if s != getattr(self, "_cur_stream", None):     # one C call per stream change, not per call
            self._check(self.lib.omb_set_stream(self._h, ctypes.c_void_p(s)), "omb_set_stream")
            self._cur_stream = s

    def _out(self, out, shape, dtype=torch.float64):
        return out if out is not None else torch.empty(shape, dtype=dtype, device=self.device)

    def _boxes_dev(self, boxes):
        if isinstance(boxes, torch.Tensor):
            return boxes
        # uint16 indices < 32768 travel as int16 (torch has no uint16 on every build)
        return torch.as_tensor(np.ascontiguousarray(boxes, dtype=np.uint16).view(np.int16), device=self.device)

    def close(self):
        if getattr(self, "_h", None):
            self.lib.omb_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        self._check(self.lib.omb_synchronize(self._h), "omb_synchronize")

    def debug_set(self, what, value):
        """omb_debug_set: ("spin_limit", polls) bounds the posterior's LDS-counter waits; ("cov_table", 0/1)
        builds K(X, X) / K(X*, X*) with the posterior's table-driven Matern transform; ("fused_chain", 0/1/2) runs
        EHVI-2D and the arg-max as separate launches / as one ticketed launch / as EHVI with per-workgroup pairs
        and the arg-max's second pass; ("argmax_passes", 1/2) runs the arg-max as one
        launch / as two; ("chol_mode", 0/1/2 [+ 4]) factors auto / by per-step launches / in one persistent launch
        [with release-acquire hand-offs];
        ("timing_stride", s) records the timing events on every s-th chain only; ("select_seq", 0/1) picks the
        Thompson selection's parallel rounds (default) / its sequential walk for B <= 64; ("boxes_kd", 0/1) runs
        omb_ehvi_boxes_k candidate-blocked (default) / one wavefront per candidate where its tables fit;
        ("posterior_all_var", 0/1) lets the fused chain skip the posterior variance of objectives the planned
        acquisition never reads (default) / compute every objective's (bit-identical values);
        ("posterior_mean_kernel", 0/1/2) computes those objectives' mean inside the posterior launch / in a kernel
        of its own after it (default) / in that kernel before it (bit-identical values); ("paths_libcos", 0/1)
        evaluates the sample paths' features with the kernel's own cosine (default) / the device library's;
        ("hvi_paths_chunk", c) evaluates a ``plan_hvi_paths`` chain in passes of c candidates (default
        ``_lib.HVI_PATHS_CHUNK``; 0: one pass; bit-identical values); ("argmax_prune", 0/1/2/3) runs the arg-max
        chain of a reference-mode EHVI-2D plan densely / in two phases, seeded by each group's best bound, from 2^16
        candidates on (default) / in two phases with the strided seed at any size / in two phases seeded by the
        bound at any size (bit-identical pair; see ``argmax_prune_stats``); ("argmax_screen", 0/1) feeds that path's
        bound fp64 means of every candidate / ``posterior_screen``'s means and margins (default; bit-identical
        pair); ("argmax_staged", 0/1) runs the seeded-by-bound path with both objectives' screen and the full bound
        for every candidate / staged (default): objective 1's screen and a bound from it alone for every candidate,
        objective 0's screen and the full bound only for those it keeps — 0 is the order for batches where
        objective 0 decides (bit-identical pair; see ``argmax_stage_stats``); ("argmax_cut", 0/1) draws the staged
        order's first list by evaluating objective 1's bound for every candidate / by one cut on the low end of its
        screened mean, solved once per call (default; bit-identical pair; see ``argmax_cut_stats``)."""
        code = getattr(_lib, "DEBUG_" + str(what).upper(), None)
        if code is None:
            raise KeyError(what)
        self._check(self.lib.omb_debug_set(self._h, code, int(value)), "omb_debug_set")

    # ------------------------------------------------------------------ GP state
    def set_gp(self, obj, X, lengthscale, variance, alpha, Linv, kernel="matern52"):
        """Upload one fitted GP (see optimobo_amd.gp.GPState) for objective ``obj``."""
        X = _dev_f64(X, self.device)
        alpha = _dev_f64(np.asarray(alpha).reshape(-1) if not isinstance(alpha, torch.Tensor) else alpha.reshape(-1),
                         self.device)
        Linv = _dev_f64(Linv, self.device)
        n, d = X.shape
        if Linv.shape != (n, n) or alpha.shape[0] != n:
            raise ValueError(f"set_gp: shapes X{tuple(X.shape)} alpha{tuple(alpha.shape)} Linv{tuple(Linv.shape)}")
        ls = np.broadcast_to(np.asarray(lengthscale, np.float64), (d,))
        self._stream()
        self._check(self.lib.omb_set_gp(self._h, obj, _KERNEL_IDS[kernel], n, d, _ptr(X), _lib.darr(ls),
                                        float(variance), _ptr(alpha), _ptr(Linv)), "omb_set_gp")
        self._gp_keep[obj] = (X, alpha, Linv)
        self.gp_info[obj] = dict(n=n, d=d, variance=float(variance), kernel=kernel)

    def set_gp_state(self, obj, state):
        if hasattr(state, "upload"):          # DeviceGPState: factorised on the device
            state.upload(self, obj)
            return
        self.set_gp(obj, state.X, state.lengthscale, state.variance, state.alpha, state.Linv, state.kernel)

    # ------------------------------------------------------------------ posterior
    def _check_width(self, Xc, obj=0):
        """The C-ABI takes no candidate width: the kernels read Xc (N, d) with the installed GP's d."""
        info = self.gp_info.get(obj)
        if Xc.dim() != 2:
            raise ValueError(f"candidates must be (N, d), got shape {tuple(Xc.shape)}")
        if info is not None and Xc.shape[1] != info["d"]:
            raise ValueError(f"candidates have {Xc.shape[1]} columns but objective {obj}'s GP has n_var={info['d']}")

    def kernel_block(self, obj, Xc, out=None):
        Xc = _dev_f64(Xc, self.device)
        self._check_width(Xc, obj)
        n = self.gp_info[obj]["n"]
        N = Xc.shape[0]
        K = self._out(out, (n, N))
        self._stream()
        self._check(self.lib.omb_kernel_block(self._h, obj, _ptr(Xc), N, _ptr(K)), "omb_kernel_block")
        return K

    def posterior(self, Xc, n_obj=None, out=None):
        """μ, σ² (n_obj, N) of objectives 0..n_obj-1 at candidates Xc (N, d)."""
        Xc = _dev_f64(Xc, self.device)
        self._check_width(Xc)
        n_obj = n_obj if n_obj is not None else len(self.gp_info)
        N = Xc.shape[0]
        mu, var = out if out is not None else (self._out(None, (n_obj, N)), self._out(None, (n_obj, N)))
        self._stream()
        self._check(self.lib.omb_posterior(self._h, n_obj, _ptr(Xc), N, _ptr(mu), _ptr(var)), "omb_posterior")
        return mu, var

    def posterior_screen(self, Xc, n_obj=None, out=None):
        """omb_posterior_screen: (μ̃, ε), each fp64 (n_obj, N) — the posterior mean with the kernel transform in
        fp32 and a rigorous margin, |μ̃ − μ| ≤ ε against ``posterior``'s μ (n_var ≤ 8).  What the arg-max chain's
        two-phase path prunes with ("argmax_screen")."""
        Xc = _dev_f64(Xc, self.device)
        self._check_width(Xc)
        n_obj = n_obj if n_obj is not None else len(self.gp_info)
        N = Xc.shape[0]
        mu, eps = out if out is not None else (self._out(None, (n_obj, N)), self._out(None, (n_obj, N)))
        self._stream()
        self._check(self.lib.omb_posterior_screen(self._h, _ptr(Xc), N, n_obj, _ptr(mu), _ptr(eps)),
                    "omb_posterior_screen")
        return mu, eps

    def posterior_screen_list(self, Xc, idx, count, obj, mu, eps):
        """omb_posterior_screen_list: ``posterior_screen`` of objective ``obj`` alone for the candidates
        ``idx[:count]`` (int32 device tensors; ``count`` one element), written in place to ``mu[idx]``, ``eps[idx]``
        (fp64 device rows of N) with ``posterior_screen``'s bits; unlisted slots are left alone."""
        Xc = _dev_f64(Xc, self.device)
        self._check_width(Xc, obj)
        N = Xc.shape[0]
        if idx.dtype != torch.int32 or count.dtype != torch.int32 or idx.numel() > N or count.numel() != 1:
            raise ValueError("posterior_screen_list: idx (<= N) and count (1) must be int32 device tensors")
        if mu.dtype != torch.float64 or eps.dtype != torch.float64 or mu.numel() != N or eps.numel() != N:
            raise ValueError("posterior_screen_list: mu and eps must be fp64 rows of N")
        if not (idx.is_contiguous() and mu.is_contiguous() and eps.is_contiguous()):
            raise ValueError("posterior_screen_list: contiguous tensors only")
        self._stream()
        self._check(self.lib.omb_posterior_screen_list(self._h, _ptr(Xc), N, _ptr(idx), _ptr(count), int(obj),
                                                       _ptr(mu), _ptr(eps)), "omb_posterior_screen_list")
        return mu, eps

    # ------------------------------------------------------------------ acquisitions
    def ehvi2d(self, mu, var, pf_sorted, r, s00, s01, mode="reference", out=None):
        N = mu.shape[1]
        pf = _dev_f64(pf_sorted, self.device)
        out = self._out(out, N)
        self._stream()
        self._check(self.lib.omb_ehvi2d(self._h, _ptr(mu), _ptr(var), mu.stride(0), N, _ptr(pf), pf.shape[0],
                                        _lib.darr(r), float(s00), float(s01), _EHVI_MODES[mode], _ptr(out)),
                    "omb_ehvi2d")
        return out

    def ehvi_mc(self, mu, var, cache, r, hv_pf, out=None, raised=None):
        """EHVI_3D's Monte-Carlo form over k = cache.shape[1] objectives (rows 0..k-1 of mu/var):
        (values (N,), raised (N,) int32); NaN and raised = 1 where pygmo would raise."""
        N = mu.shape[1]
        cache = _dev_f64(cache, self.device)
        if cache.dim() != 2 or not 2 <= cache.shape[1] <= mu.shape[0] or len(r) != cache.shape[1]:
            raise ValueError(f"ehvi_mc: cache {tuple(cache.shape)}, r of {len(r)}, mu {tuple(mu.shape)} disagree on k")
        out = self._out(out, N)
        raised = self._out(raised, N, torch.int32)
        self._stream()
        self._check(self.lib.omb_ehvi_mc(self._h, cache.shape[1], _ptr(mu), _ptr(var), mu.stride(0), N, _ptr(cache),
                                         cache.shape[0], _lib.darr(r), float(hv_pf), _ptr(out), _ptr(raised)),
                    "omb_ehvi_mc")
        return out, raised

    def ehvi3d_mc(self, mu, var, cache, r, hv_pf, out=None, raised=None):
        N = mu.shape[1]
        cache = _dev_f64(cache, self.device)
        out = self._out(out, N)
        raised = self._out(raised, N, torch.int32)
        self._stream()
        self._check(self.lib.omb_ehvi3d_mc(self._h, _ptr(mu), _ptr(var), mu.stride(0), N, _ptr(cache), cache.shape[0],
                                           _lib.darr(r), float(hv_pf), _ptr(out), _ptr(raised)), "omb_ehvi3d_mc")
        return out, raised

    def ehvi_boxes(self, mu, var, coords, boxes, out=None, kd=None):
        """Exact EHVI over a box decomposition (optimobo_amd.pareto.box_decomposition).  kd: None picks the
        entry by k; True / False force omb_ehvi_boxes_k (any 2 ≤ k ≤ 8) / omb_ehvi_boxes (k ≤ 3)."""
        k, N = mu.shape
        coords = _dev_f64(coords, self.device)
        boxes = self._boxes_dev(boxes)
        out = self._out(out, N)
        self._stream()
        # k = 2, 3: one wavefront per candidate; k >= 4: the candidate-blocked k-D kernel (omb_ehvi_boxes_k)
        fn = "omb_ehvi_boxes_k" if (k > 3 if kd is None else kd) else "omb_ehvi_boxes"
        self._check(getattr(self.lib, fn)(self._h, k, _ptr(mu), _ptr(var), mu.stride(0), N, _ptr(coords),
                                          coords.shape[1], _ptr(boxes), boxes.shape[0], _ptr(out)), fn)
        return out

    def hvi_boxes(self, y, coords, boxes, out=None):
        """omb_hvi_boxes: the hypervolume improvement Σ_b Π_j (hi_bj − max(y_j, lo_bj))⁺ of the N points y (k, N)
        (objective-major, unit column stride) over a box decomposition (optimobo_amd.pareto.box_decomposition)
        → (N,).  A point's value is bitwise the same wherever it stands in whatever batch."""
        if not isinstance(y, torch.Tensor) or y.dim() != 2 or y.dtype != torch.float64 or y.device != self.device \
                or (y.shape[1] > 1 and y.stride(1) != 1):
            raise ValueError(f"hvi_boxes: y must be a (k, N) fp64 tensor on {self.device} with unit column stride")
        k, N = y.shape
        coords = _dev_f64(coords, self.device)
        if coords.dim() != 2 or coords.shape[0] != k:
            raise ValueError(f"hvi_boxes: grid {tuple(coords.shape)} for k={k} objectives")
        boxes = self._boxes_dev(boxes)
        # a device list is read as it is: (B, 2k) 16-bit indices, or the kernel would walk past its end
        if boxes.dim() != 2 or boxes.shape[1] != 2 * k or boxes.element_size() != 2 or boxes.is_floating_point() \
                or boxes.device != self.device or not boxes.is_contiguous():
            raise ValueError(f"hvi_boxes: the box list must be a contiguous (B, {2 * k}) 16-bit integer tensor on "
                             f"{self.device}, got {tuple(boxes.shape)} {boxes.dtype} on {boxes.device}")
        if out is None:
            out = self._out(None, N)
        elif out.dtype != torch.float64 or out.device != self.device or out.numel() < N or not out.is_contiguous():
            raise ValueError(f"hvi_boxes: out must be a contiguous fp64 tensor of at least {N} values on {self.device}")
        self._stream()
        self._check(self.lib.omb_hvi_boxes(self._h, k, _ptr(y), y.stride(0) if k > 1 else N, N, _ptr(coords),
                                           coords.shape[1], _ptr(boxes), boxes.shape[0], _ptr(out)), "omb_hvi_boxes")
        return out

    @staticmethod
    def _box_lists_host(coords, box_off, boxes, what):
        """(coords (S, k, C) f64, box_off (S + 1,) int32, boxes (ΣB, 2k) uint16) as C-contiguous numpy, shapes held
        against each other (optimobo_amd.pareto.pack_box_lists builds them)."""
        c = np.ascontiguousarray(coords, dtype=np.float64)
        o = np.ascontiguousarray(box_off, dtype=np.int32).reshape(-1)
        b = np.ascontiguousarray(boxes, dtype=np.uint16)
        if c.ndim != 3 or o.shape[0] != c.shape[0] + 1 or b.ndim != 2 or b.shape[1] != 2 * c.shape[1] \
                or (o.shape[0] and int(o[-1]) != b.shape[0]):
            raise ValueError(f"{what}: grids {c.shape}, offsets {o.shape} and box lists {b.shape} are not "
                             "(S, k, C), (S + 1,) and (box_off[S], 2k)")
        return c, o, b

    def hvi_paths(self, y, coords, box_off, boxes, out=None):
        """omb_hvi_paths: the mean over S sampled fronts of the hypervolume improvement of every candidate's path
        values — y (k, S, N) as ``paths_eval`` returns them (rows may be pitched: y[j, s] at pitch ld ≥ N), list s =
        rows box_off[s]..box_off[s+1] of boxes over the grid coords[s] (optimobo_amd.pareto.pack_box_lists) → (N,).
        At most 16 paths (one path install).  k = 1 with ``pareto.threshold_lists`` is the noisy EI's integrand."""
        c, o, b = self._box_lists_host(coords, box_off, boxes, "hvi_paths")
        S, k, C = c.shape
        if not isinstance(y, torch.Tensor) or y.dtype != torch.float64 or y.device != self.device or y.dim() != 3 \
                or tuple(y.shape[:2]) != (k, S) or (y.shape[2] > 1 and y.stride(2) != 1) \
                or y.stride(0) != S * y.stride(1) or y.stride(1) < y.shape[2]:
            raise ValueError(f"hvi_paths: y must be a ({k}, {S}, N) fp64 tensor on {self.device} with unit column "
                             "stride and evenly pitched rows")
        N = y.shape[2]
        if out is None:
            out = self._out(None, N)
        elif out.dtype != torch.float64 or out.device != self.device or out.numel() < N or not out.is_contiguous():
            raise ValueError(f"hvi_paths: out must be a contiguous fp64 tensor of at least {N} values on {self.device}")
        cd = torch.as_tensor(c, device=self.device)
        bd = self._boxes_dev(b)
        self._stream()
        self._check(self.lib.omb_hvi_paths(self._h, k, S, _ptr(y), y.stride(1), N, _ptr(cd), C, _lib.host_ptr(o),
                                           _ptr(bd), _ptr(out)), "omb_hvi_paths")
        return out

    def hvi_paths_con(self, y, n_con, coords, box_off, boxes, eta=0.0, violation=False, out=None, per_path=False):
        """omb_hvi_paths_con: ``hvi_paths`` under constraints through sample paths — y (k + n_con, S, N) as
        ``paths_eval`` returns it over the objectives and then the constraint models (g ≤ 0 feasible); path s of a
        candidate counts with the weight w_s = Π_j ω(g_js): the indicator at ``eta`` = 0, the sigmoid of −g/eta above.
        → (N,) the mean of u_s = t_s·w_s; with ``per_path`` → (mean (N,), u (S, N)).  ``violation`` (eta = 0): an
        infeasible path scores −(its total violation) in place of 0.  At n_con = 0 the mean is bitwise ``hvi_paths``."""
        c, o, b = self._box_lists_host(coords, box_off, boxes, "hvi_paths_con")
        S, k, C = c.shape
        n_con = int(n_con)
        if not isinstance(y, torch.Tensor) or y.dtype != torch.float64 or y.device != self.device or y.dim() != 3 \
                or n_con < 0 or tuple(y.shape[:2]) != (k + n_con, S) or (y.shape[2] > 1 and y.stride(2) != 1) \
                or y.stride(0) != S * y.stride(1) or y.stride(1) < y.shape[2]:
            raise ValueError(f"hvi_paths_con: y must be a ({k} + n_con, {S}, N) fp64 tensor on {self.device} with unit "
                             "column stride and evenly pitched rows")
        N, ld = y.shape[2], y.stride(1)
        if out is None:
            out = self._out(None, N)
        elif out.dtype != torch.float64 or out.device != self.device or out.numel() < N or not out.is_contiguous():
            raise ValueError(f"hvi_paths_con: out must be a contiguous fp64 tensor of at least {N} values on "
                             f"{self.device}")
        u = torch.empty((S, ld), dtype=torch.float64, device=self.device) if per_path else None
        cd = torch.as_tensor(c, device=self.device)
        bd = self._boxes_dev(b)
        self._stream()
        self._check(self.lib.omb_hvi_paths_con(self._h, k, S, n_con, _ptr(y), ld, N, _ptr(cd), C, _lib.host_ptr(o),
                                               _ptr(bd), float(eta), _lib.CON_VIOLATION if violation else 0, _ptr(out),
                                               None if u is None else _ptr(u)), "omb_hvi_paths_con")
        return (out, u[:, :N]) if per_path else out

    def _point_sets(self, what, Y, S):
        """Y (k, N) with S = 1 or (k, S, N), rows possibly pitched → (Y (k, S, N), k, S, N, ld) in the layout of
        omb_nondominated / omb_hypervolume: row j·S + s at pitch ld."""
        if not isinstance(Y, torch.Tensor) or Y.dtype != torch.float64 or Y.device != self.device:
            raise ValueError(f"{what}: Y must be an fp64 tensor on {self.device}")
        S = int(S)
        if Y.dim() == 2 and S == 1:
            Y = Y[:, None, :]
        if Y.dim() != 3 or Y.shape[1] != S and S != 1:
            raise ValueError(f"{what}: Y {tuple(Y.shape)} is not (k, N) with S = 1 or (k, S, N)")
        k, S, N = Y.shape
        # row j·S + s at pitch ld: the set stride where there are several sets, else the coordinate stride
        ld = Y.stride(1) if S > 1 else (Y.stride(0) if k > 1 else max(N, 1))
        if N > 0 and ((N > 1 and Y.stride(2) != 1) or ld < N or (S > 1 and k > 1 and Y.stride(0) != S * ld)):
            raise ValueError(f"{what}: Y needs unit column stride and evenly pitched rows (row j·S + s at pitch ld)")
        ld = max(int(ld), N, 1) if N == 0 else int(ld)
        return Y, k, S, N, ld

    def _set_mask(self, what, mask, S, N):
        """A bool / uint8 mask (S, ldm ≥ N) — (N,) with S = 1 — on the device with unit column stride →
        (uint8 view, ldm); (None, N) for no mask."""
        if mask is None:
            return None, max(N, 1)
        if isinstance(mask, torch.Tensor) and mask.dtype == torch.bool:
            mask = mask.view(torch.uint8)
        if isinstance(mask, torch.Tensor) and mask.dim() == 1 and S == 1:
            mask = mask[None, :]
        if not isinstance(mask, torch.Tensor) or mask.dtype != torch.uint8 or mask.device != self.device \
                or mask.dim() != 2 or mask.shape[0] != S or mask.shape[1] < N \
                or (mask.shape[1] > 1 and mask.stride(1) != 1) or (S > 1 and mask.stride(0) < N):
            raise ValueError(f"{what}: mask must be a bool or uint8 ({S}, ldm >= {N}) tensor on {self.device} with "
                             "unit column stride")
        return mask, int(mask.stride(0)) if S > 1 else max(mask.shape[1], N, 1)

    def _ref_point(self, what, ref, k):
        r = np.ascontiguousarray(np.asarray(ref.detach().cpu() if isinstance(ref, torch.Tensor) else ref,
                                            dtype=np.float64).reshape(-1))
        if r.size != k:
            raise ValueError(f"{what}: the reference point has {r.size} coordinates for {k} objectives")
        return r

    def hypervolume(self, Y, ref, S=1, mask=None):
        """omb_hypervolume: the exact hypervolume (minimisation) that each of S independent point sets dominates
        below the reference point ``ref`` (k host values) — Y (k, N) with S = 1 or (k, S, N), as ``nondominated``
        takes it; ``mask`` (S, N) bool / uint8 (``nondominated``'s, say) picks the rows of every set, None takes all
        → (S,) fp64 on the device.  A row counts when every coordinate is finite and < ref_j; the rows need not be
        non-dominated or distinct; a set without such a row has hypervolume 0.0.  The result is bitwise the same
        whatever the pitch, the set's slot, the order of the rows and the number of dropped ones.  ``OMBError`` with
        code ``OMB_EUNSUP`` for a set with more than ``_lib.HV_POINTS`` counted rows or a call above
        ``_lib.HV_MAX_WORK`` point tests (``pareto.hypervolume`` has no such bound).  The call synchronises the
        stream (it reads the grid sizes to size its second launch)."""
        Y, k, S, N, ld = self._point_sets("hypervolume", Y, S)
        m, ldm = self._set_mask("hypervolume", mask, S, N)
        r = self._ref_point("hypervolume", ref, k)
        hv = torch.empty(S, dtype=torch.float64, device=self.device)
        self._stream()
        self._check(self.lib.omb_hypervolume(self._h, k, S, _ptr(Y), ld, N, None if m is None else _ptr(m),
                                             max(ldm, N), r.ctypes.data_as(_lib._dp), _ptr(hv)), "omb_hypervolume")
        return hv

    def hypervolume_contributions(self, Y, ref, mask=None):
        """omb_hypervolume_contrib: one set Y (k, N) (``mask`` (N,) bool / uint8 or None) → (hv (1,) fp64,
        contributions (N,) fp64) on the device: contributions[i] = HV(set) − HV(set without row i).  Exactly 0.0 for
        a row that does not count (masked out, a coordinate not finite or ≥ ref_j), for a duplicate and for a row
        that another counted row dominates; ``hv`` is ``hypervolume``'s value, bit for bit.  The row to drop when
        an archive is truncated is the counted row with the least contribution.  Refusals and synchronisation as
        ``hypervolume``; the work is (n + 1) times its."""
        Y, k, S, N, ld = self._point_sets("hypervolume_contributions", Y, 1)
        if S != 1:
            raise ValueError("hypervolume_contributions: one set, Y (k, N)")
        m, _ = self._set_mask("hypervolume_contributions", mask, 1, N)
        r = self._ref_point("hypervolume_contributions", ref, k)
        hv = torch.empty(1, dtype=torch.float64, device=self.device)
        contrib = torch.empty(max(N, 1), dtype=torch.float64, device=self.device)
        self._stream()
        self._check(self.lib.omb_hypervolume_contrib(self._h, k, _ptr(Y), ld, N, None if m is None else _ptr(m),
                                                     r.ctypes.data_as(_lib._dp), _ptr(hv), _ptr(contrib)),
                    "omb_hypervolume_contrib")
        return hv, contrib[:N]

    def nondominated(self, Y, S=1, out=None):
        """omb_nondominated: the non-dominated points (minimisation) of S independent point sets — Y (k, N) with
        S = 1 (the layout of ``posterior``'s mean) or (k, S, N) as ``paths_eval`` returns it (rows may be pitched) →
        (mask (S, N) bool, counts (S,) int64), both on the device.  mask[s, i] is True when no point of set s
        dominates point i and none of its coordinates is NaN; duplicates are all kept, −0.0 equals +0.0, ±inf are
        ordinary values.  On NaN-free input it is ``pareto.nondominated_mask``, bit for bit.  ``out``: a uint8
        (S, ldm ≥ N) tensor with unit column stride to take the mask (columns past N stay untouched).  The call
        synchronises the stream (it reads the sieve's survivor counts to size its later passes)."""
        Y, k, S, N, ld = self._point_sets("nondominated", Y, S)
        if out is None:
            out = torch.empty((S, N), dtype=torch.uint8, device=self.device)
        elif not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.device != self.device \
                or out.dim() != 2 or out.shape[0] != S or out.shape[1] < N or (out.shape[1] > 1 and out.stride(1) != 1) \
                or (S > 1 and out.stride(0) < N):
            raise ValueError(f"nondominated: out must be a uint8 ({S}, ldm >= {N}) tensor on {self.device} with unit "
                             "column stride")
        ldm = out.stride(0) if S > 1 else max(out.shape[1], 1)
        counts = torch.empty(S, dtype=torch.int64, device=self.device)
        self._stream()
        self._check(self.lib.omb_nondominated(self._h, k, S, _ptr(Y), int(ld), N, _ptr(out), int(ldm), _ptr(counts)),
                    "omb_nondominated")
        return out[:, :N].view(torch.bool), counts

    def nondominated_stats(self):
        """omb_nondominated_stats: the sieve of the last ``nondominated`` call → the largest set's survivors after
        each of its tile passes (a list of 1 to 4 counts; empty before any call or after an empty one)."""
        surv = (ctypes.c_int64 * 5)()
        rounds = ctypes.c_int()
        self._check(self.lib.omb_nondominated_stats(self._h, surv, ctypes.byref(rounds)), "omb_nondominated_stats")
        return [int(v) for v in surv[:rounds.value]]

    def argmax_prune_stats(self):
        """omb_argmax_prune_stats: the last ``eval_argmax`` / ``eval_argmax_sobol`` call → (two_phase, seed,
        survivors): whether it took the two-phase path, the candidates of its seed (one per 256, or every 16th
        under "argmax_prune" 2) and those past the seed that its bound kept (the call's own once its result has been
        waited for).  (False, 0, 0) after a dense call."""
        st = (ctypes.c_int64 * 3)()
        self._check(self.lib.omb_argmax_prune_stats(self._h, st), "omb_argmax_prune_stats")
        return bool(st[0]), int(st[1]), int(st[2])

    def argmax_stage_stats(self):
        """omb_argmax_stage_stats: the same call → (staged, |A|, |B|): whether it took the staged order
        ("argmax_staged"), the candidates past the seed that objective 1's bound kept, and those of them that the
        full bound kept (``argmax_prune_stats``'s survivors).  (False, 0, 0) otherwise."""
        st = (ctypes.c_int64 * 3)()
        self._check(self.lib.omb_argmax_stage_stats(self._h, st), "omb_argmax_stage_stats")
        return bool(st[0]), int(st[1]), int(st[2])

    def argmax_cut_stats(self):
        """omb_argmax_cut_stats: the same call → (cut, m*, τ₀, ubm1(m*)): whether the staged order drew its first
        list by the cut ("argmax_cut"), the cut on the low end of objective 1's screened mean (+inf: nothing could
        be dropped), the seed's best value and objective 1's bound at m* (NaN where m* is +inf).
        (False, 0.0, 0.0, 0.0) otherwise."""
        st = (ctypes.c_double * 4)()
        self._check(self.lib.omb_argmax_cut_stats(self._h, st), "omb_argmax_cut_stats")
        return bool(st[0]), float(st[1]), float(st[2]), float(st[3])

    def hvpoi(self, mu, var, cells, out=None):
        N = mu.shape[1]
        cells = _dev_f64(cells, self.device)
        out = self._out(out, N)
        self._stream()
        self._check(self.lib.omb_hvpoi(self._h, _ptr(mu), _ptr(var), mu.stride(0), N, _ptr(cells), cells.shape[0],
                                       _ptr(out)), "omb_hvpoi")
        return out

    def expdec(self, mu, var, cache, scal_id, params, weights, ideal, max_point, agg_min, out=None):
        k, N = mu.shape
        cache = _dev_f64(cache, self.device)
        out = self._out(out, N)
        self._stream()
        self._check(self.lib.omb_expdec(self._h, k, _ptr(mu), _ptr(var), mu.stride(0), N, _ptr(cache), cache.shape[0],
                                        int(scal_id), _lib.darr(params), _lib.darr(weights), _lib.darr(ideal),
                                        _lib.darr(max_point), float(agg_min), _ptr(out)), "omb_expdec")
        return out

    def ei(self, mu, var, best, var_eps=0.0, out=None):
        mu = mu.reshape(-1)
        var = var.reshape(-1)
        N = mu.shape[0]
        out = self._out(out, N)
        self._stream()
        self._check(self.lib.omb_ei(self._h, _ptr(mu), _ptr(var), N, float(best), float(var_eps), _ptr(out)), "omb_ei")
        return out

    def ei_ext(self, kind, mu, var, best, var_eps=0.0, pof_eps=0.0, out=None):
        """EI family over rows 0..k-1 of (mu, var): kind "plain" | "pareto" (KEEP) | "constrained" (cParEGO)."""
        k, N = mu.shape
        out = self._out(out, N)
        self._stream()
        self._check(self.lib.omb_ei_ext(self._h, _EI_KINDS[kind], k, _ptr(mu), _ptr(var), mu.stride(0), N,
                                        float(best), float(var_eps), float(pof_eps), _ptr(out)), "omb_ei_ext")
        return out

    def feasibility(self, mu, var, pof_eps=1e-5, acq=None, out=None):
        """omb_feasibility: the probability of feasibility F = Π_j Φ(−μ_j / sqrt(σ²_j + pof_eps)) over the rows of
        (mu, var) (c, N) — constraint models, feasible where g ≤ 0 — times ``acq`` (N,) when given (``out`` may be
        ``acq``)."""
        c, N = mu.shape
        out = self._out(out, N)
        self._stream()
        self._check(self.lib.omb_feasibility(self._h, c, _ptr(mu), _ptr(var), mu.stride(0), N, float(pof_eps),
                                             _ptr(acq) if acq is not None else None, _ptr(out)), "omb_feasibility")
        return out

    # log-space forms: finite where the linear values above are exactly 0.0 (include/optimobo_hip.h)
    def log_ei(self, mu, var, best, var_eps=0.0, pof_eps=0.0, kind="plain", out=None):
        """omb_log_ei: log EI over rows 0..k-1 of (mu, var) — kind "plain" (k = 1; 1-D moments are taken as one
        row) or "constrained" (rows 1.. are constraint models); "pareto" has no logarithm (OMB_EUNSUP)."""
        if mu.dim() == 1:
            mu, var = mu.reshape(1, -1), var.reshape(1, -1)
        k, N = mu.shape
        out = self._out(out, N)
        self._stream()
        self._check(self.lib.omb_log_ei(self._h, _EI_KINDS[kind], k, _ptr(mu), _ptr(var), mu.stride(0), N,
                                        float(best), float(var_eps), float(pof_eps), _ptr(out)), "omb_log_ei")
        return out

    def log_ehvi_boxes(self, mu, var, coords, boxes, out=None):
        """omb_log_ehvi_boxes: the logarithm of ``ehvi_boxes`` (2 ≤ k ≤ 8; one kernel for every k)."""
        k, N = mu.shape
        coords = _dev_f64(coords, self.device)
        boxes = self._boxes_dev(boxes)
        out = self._out(out, N)
        self._stream()
        self._check(self.lib.omb_log_ehvi_boxes(self._h, k, _ptr(mu), _ptr(var), mu.stride(0), N, _ptr(coords),
                                                coords.shape[1], _ptr(boxes), boxes.shape[0], _ptr(out)),
                    "omb_log_ehvi_boxes")
        return out

    def log_feasibility(self, mu, var, pof_eps=1e-5, acq=None, out=None):
        """omb_log_feasibility: log F = Σ_j log Φ(−μ_j / sqrt(σ²_j + pof_eps)) over the rows of (mu, var) (c, N),
        plus ``acq`` (N,) — a log acquisition — when given (``out`` may be ``acq``)."""
        c, N = mu.shape
        out = self._out(out, N)
        self._stream()
        self._check(self.lib.omb_log_feasibility(self._h, c, _ptr(mu), _ptr(var), mu.stride(0), N, float(pof_eps),
                                                 _ptr(acq) if acq is not None else None, _ptr(out)),
                    "omb_log_feasibility")
        return out

    def mes(self, mu, var, ystar, out=None):
        """omb_mes: max-value entropy search over rows 0..k-1 of (mu, var) (1-D moments are taken as one row) and
        the sampled minima ``ystar`` (k, S): Σ_j mean_s a((μ_j − y*_js)/σ_j), a(γ) = γφ/(2Φ) − log Φ."""
        if mu.dim() == 1:
            mu, var = mu.reshape(1, -1), var.reshape(1, -1)
        k, N = mu.shape
        ystar = _dev_f64(ystar, self.device).reshape(k, -1)
        out = self._out(out, N)
        self._stream()
        self._check(self.lib.omb_mes(self._h, k, _ptr(mu), _ptr(var), mu.stride(0), N, _ptr(ystar), ystar.shape[1],
                                     _ptr(out)), "omb_mes")
        return out

    def argmax_dev(self, vals, offset=0, out=None):
        out = self._out(out, 2)
        self._stream()
        self._check(self.lib.omb_argmax_dev(self._h, _ptr(vals), vals.numel(), int(offset), _ptr(out)), "omb_argmax_dev")
        return out

    def argmax(self, vals, offset=0):
        v = ctypes.c_double()
        i = ctypes.c_int64()
        self._stream()
        self._check(self.lib.omb_argmax(self._h, _ptr(vals), vals.numel(), int(offset), ctypes.byref(v),
                                        ctypes.byref(i)), "omb_argmax")
        return v.value, i.value

    # ------------------------------------------------------------------ fused chain (plans)
    def _plan(self, fn, *args, mode=None):
        self._stream()
        self.plan_kind = None          # a failed plan call leaves no plan
        self.plan_is_log = False       # every plan starts linear (omb_plan_log's flag is cleared)
        self._check(getattr(self.lib, fn)(self._h, *args), fn)
        self.plan_kind = (fn, mode)

    # plans omb_eval_grad differentiates (include/optimobo_hip.h); EHVI-2D in "sigma" mode is not one
    _GRAD_PLANS = ("omb_plan_ei", "omb_plan_ei_ext", "omb_plan_ehvi2d", "omb_plan_ehvi_boxes", "omb_plan_ehvi_boxes_k",
                   "omb_plan_mes")

    def plan_has_gradient(self):
        """True when the plan last set through this context is one omb_eval_grad differentiates."""
        if self.plan_kind is None:
            return False
        fn, mode = self.plan_kind
        if self.plan_is_log and fn in ("omb_plan_ehvi_boxes", "omb_plan_ehvi_boxes_k"):
            return False               # the log exact EHVI has no analytic gradient yet (log EI has)
        return fn in self._GRAD_PLANS and mode != "sigma"

    def plan_ehvi2d(self, pf_sorted, r, s00, s01, mode="reference"):
        pf = np.ascontiguousarray(pf_sorted, dtype=np.float64).reshape(-1, 2)
        self._plan("omb_plan_ehvi2d", _lib.host_ptr(pf), pf.shape[0], _lib.darr(r), float(s00), float(s01),
                   _EHVI_MODES[mode], mode=mode)

    def plan_ehvi_mc(self, cache, r, hv_pf):
        """EHVI_3D's Monte-Carlo form for k = cache.shape[1] objectives (cache (M, k), r (k,))."""
        c = np.ascontiguousarray(cache, dtype=np.float64)
        if c.ndim != 2 or len(r) != c.shape[1]:
            raise ValueError(f"plan_ehvi_mc: cache {c.shape} and r of {len(r)} disagree on k")
        self._plan("omb_plan_ehvi_mc", c.shape[1], _lib.host_ptr(c), c.shape[0], _lib.darr(r), float(hv_pf))

    def plan_ehvi3d_mc(self, cache, r, hv_pf):
        c = np.ascontiguousarray(cache, dtype=np.float64).reshape(-1, 3)
        self._plan("omb_plan_ehvi3d_mc", _lib.host_ptr(c), c.shape[0], _lib.darr(r), float(hv_pf))

    def plan_ehvi_boxes(self, coords, boxes):
        c = np.ascontiguousarray(coords, dtype=np.float64)
        b = np.ascontiguousarray(boxes, dtype=np.uint16)
        fn = "omb_plan_ehvi_boxes" if c.shape[0] <= 3 else "omb_plan_ehvi_boxes_k"
        self._plan(fn, c.shape[0], _lib.host_ptr(c), c.shape[1], _lib.host_ptr(b), b.shape[0])

    def plan_hvpoi(self, cells):
        c = np.ascontiguousarray(cells, dtype=np.float64).reshape(-1, 2, 2)
        self._plan("omb_plan_hvpoi", _lib.host_ptr(c), c.shape[0])

    def plan_expdec(self, cache, scal_id, params, weights, ideal, max_point, agg_min):
        c = np.ascontiguousarray(cache, dtype=np.float64)
        self._plan("omb_plan_expdec", c.shape[1], _lib.host_ptr(c), c.shape[0], int(scal_id), _lib.darr(params),
                   _lib.darr(weights), _lib.darr(ideal), _lib.darr(max_point), float(agg_min))

    def plan_ei(self, best, var_eps=0.0):
        self._plan("omb_plan_ei", float(best), float(var_eps))

    def plan_ei_ext(self, kind, k, best, var_eps=0.0, pof_eps=0.0):
        self._plan("omb_plan_ei_ext", _EI_KINDS[kind], int(k), float(best), float(var_eps), float(pof_eps))

    def plan_mes(self, ystar):
        """omb_plan_mes: ``mes`` as the chain's plan over objectives 0..k-1, ystar (k, S) on the host (a non-finite
        entry is refused and leaves no plan)."""
        y = np.ascontiguousarray(ystar, dtype=np.float64)
        if y.ndim != 2:
            raise ValueError(f"plan_mes: ystar {y.shape} is not (k, S)")
        self._plan("omb_plan_mes", y.shape[0], y.shape[1], _lib.host_ptr(y))

    def plan_hvi_paths(self, coords, box_off, boxes):
        """omb_plan_hvi_paths: ``hvi_paths`` as the chain's plan over objectives 0..k-1 — every ``eval`` evaluates the
        installed sample paths (``paths_set`` with S = the number of lists; at most 16) in place of the posterior, in
        passes of ``_lib.HVI_PATHS_CHUNK`` candidates, and averages their improvement over the S lists.
        ``plan_has_gradient()`` is False; ``plan_constraints`` and ``plan_log`` refuse the plan (OMB_EUNSUP).  A
        state change after ``paths_set`` makes ``eval`` fail with OMB_ESTATE."""
        c, o, b = self._box_lists_host(coords, box_off, boxes, "plan_hvi_paths")
        self._plan("omb_plan_hvi_paths", c.shape[1], c.shape[0], _lib.host_ptr(c), c.shape[2], _lib.host_ptr(o),
                   _lib.host_ptr(b))

    def plan_hvi_paths_con(self, n_con, coords, box_off, boxes, eta=0.0):
        """omb_plan_hvi_paths_con: ``hvi_paths_con`` (no violation score) as the chain's plan — every ``eval``
        evaluates the installed sample paths of slots 0..k+n_con-1 (objectives, then constraint models) and averages
        the weighted improvement over the S lists.  The plan carries its own constraints: ``plan_constraints`` and
        ``plan_log`` refuse it (OMB_EUNSUP), ``plan_has_gradient()`` is False."""
        c, o, b = self._box_lists_host(coords, box_off, boxes, "plan_hvi_paths_con")
        self._plan("omb_plan_hvi_paths_con", c.shape[1], c.shape[0], int(n_con), float(eta), _lib.host_ptr(c),
                   c.shape[2], _lib.host_ptr(o), _lib.host_ptr(b))

    def plan_constraints(self, n_con, pof_eps=1e-5):
        """omb_plan_constraints: the plan that is set treats objective slots k..k+n_con-1 as constraint models
        (g ≤ 0 feasible) and weights its acquisition by their probability of feasibility.  Every plan_* call clears
        this, so it comes after the plan; n_con = 0 clears it too.  A failed call changes nothing."""
        self._stream()
        self._check(self.lib.omb_plan_constraints(self._h, int(n_con), float(pof_eps)), "omb_plan_constraints")

    def plan_log(self, on=True):
        """omb_plan_log: the plan that is set returns the logarithm of its acquisition (EI plain / constrained, exact
        EHVI over boxes; OMB_EUNSUP for the others), and ``plan_constraints`` adds log F in place of multiplying by
        F.  Every plan_* call clears it; it may come before or after ``plan_constraints``.  A failed call changes
        nothing."""
        self._stream()
        self._check(self.lib.omb_plan_log(self._h, int(on)), "omb_plan_log")
        self.plan_is_log = bool(on)

    def set_sobol(self, d, lo, hi, seed=None, scramble=True, state=None):
        """Device Sobol' engine = scipy qmc.Sobol(d, scramble=scramble, seed=seed) over [lo, hi]."""
        from .sobol import engine_state
        sv, shift, bits = state if state is not None else engine_state(d, seed, scramble)
        lo = np.broadcast_to(np.asarray(lo, np.float64), (d,))
        hi = np.broadcast_to(np.asarray(hi, np.float64), (d,))
        self._stream()
        self._check(self.lib.omb_set_sobol(self._h, d, bits, _lib.host_ptr(sv), _lib.host_ptr(shift), _lib.darr(lo),
                                           _lib.darr(hi)), "omb_set_sobol")
        self.sobol_dim = d

    def sobol(self, start, N, out=None):
        out = self._out(out, (N, self.sobol_dim))
        self._stream()
        self._check(self.lib.omb_sobol(self._h, int(start), int(N), _ptr(out)), "omb_sobol")
        return out

    def eval(self, Xc, out=None):
        Xc = _dev_f64(Xc, self.device)
        self._check_width(Xc)
        N = Xc.shape[0]
        out = self._out(out, N)
        self._stream()
        self._check(self.lib.omb_eval(self._h, _ptr(Xc), N, _ptr(out)), "omb_eval")
        return out

    def posterior_grad(self, Xc, n_obj=None):
        """omb_posterior_grad: (mu, var (n_obj, N), dmu, dvar (n_obj, N, d)) — the posterior moments of objectives
        0..n_obj-1 at Xc (N, d), bitwise ``posterior``'s, and their gradients with respect to each candidate."""
        Xc = _dev_f64(Xc, self.device)
        self._check_width(Xc)
        n_obj = n_obj if n_obj is not None else len(self.gp_info)
        N, d = Xc.shape
        mu = torch.empty((n_obj, N), dtype=torch.float64, device=self.device)
        var = torch.empty_like(mu)
        dmu = torch.empty((n_obj, N, d), dtype=torch.float64, device=self.device)
        dvar = torch.empty_like(dmu)
        self._stream()
        self._check(self.lib.omb_posterior_grad(self._h, int(n_obj), _ptr(Xc), N, _ptr(mu), _ptr(var), _ptr(dmu),
                                                _ptr(dvar)), "omb_posterior_grad")
        return mu, var, dmu, dvar

    def eval_grad(self, Xc):
        """omb_eval_grad: (vals (N,), grad (N, d)) — the plan's acquisition at Xc (N, d), bitwise ``eval``'s, and
        its gradient with respect to each candidate.  OMBError (OMB_EUNSUP) for a plan without a gradient."""
        Xc = _dev_f64(Xc, self.device)
        self._check_width(Xc)
        N, d = Xc.shape
        vals = torch.empty(N, dtype=torch.float64, device=self.device)
        grad = torch.empty((N, d), dtype=torch.float64, device=self.device)
        self._stream()
        self._check(self.lib.omb_eval_grad(self._h, _ptr(Xc), N, _ptr(vals), _ptr(grad)), "omb_eval_grad")
        return vals, grad

    def eval_argmax(self, Xc, offset=0, out=None):
        Xc = _dev_f64(Xc, self.device)
        self._check_width(Xc)
        out = self._out(out, 2)
        self._stream()
        self._check(self.lib.omb_eval_argmax(self._h, _ptr(Xc), Xc.shape[0], int(offset), _ptr(out)),
                    "omb_eval_argmax")
        return out

    def eval_argmax_sobol(self, start, N, out=None):
        out = self._out(out, 2)
        self._stream()
        self._check(self.lib.omb_eval_argmax_sobol(self._h, int(start), int(N), _ptr(out)), "omb_eval_argmax_sobol")
        return out

    # ------------------------------------------------------------------ GP fit on the device
    def gp_lml_grad(self, X, y, lengthscale, variance, noise=0.0, kernel="matern52", noise_grad=False):
        """GPy's exact-inference log marginal likelihood at (σ_f², ℓ, σ_n²), its gradient w.r.t.
        (log σ_f², log ℓ_1..d) and jitchol's extra jitter: (lml, grad (d+1,), jitter).  ``noise_grad=True``
        (omb_gp_lml_grad_noise) appends ∂/∂log σ_n² = ½ σ_n² (αᵀα − tr Ky⁻¹): grad (d+2,), the rest bitwise the
        same."""
        X = _dev_f64(X, self.device)
        y = _dev_f64(y, self.device).reshape(-1)
        n, d = X.shape
        if y.shape[0] != n:
            raise ValueError(f"gp_lml_grad: y has {y.shape[0]} values for {n} inputs")
        ls = np.broadcast_to(np.asarray(lengthscale, np.float64), (d,))
        kid = _KERNEL_IDS[kernel]
        lml, jit = ctypes.c_double(), ctypes.c_double()
        grad = (ctypes.c_double * (d + 2 if noise_grad else d + 1))()
        name = "omb_gp_lml_grad_noise" if noise_grad else "omb_gp_lml_grad"
        self._stream()
        self._check(getattr(self.lib, name)(self._h, kid, n, d, _ptr(X), _ptr(y), _lib.darr(ls), float(variance),
                                            float(noise), ctypes.byref(lml), grad, ctypes.byref(jit)), name)
        return lml.value, np.array(grad[:]), jit.value

    def gp_lml_grad_batch(self, X, ys, lengthscales, variances, noise=0.0, kernel="matern52", noise_grad=False):
        """omb_gp_lml_grad_batch: k ≤ 4 GPs on the same inputs in one call — (lml (k,), grad (k, d+1),
        jitter (k,), status (k,)); status[p] is 0 or OMB_ENOTPD for problem p.  ``noise_grad=True``
        (omb_gp_lml_grad_noise_batch): ``noise`` is a scalar or one value per problem and grad is (k, d+2),
        the last entry ∂/∂log σ_n²."""
        X = _dev_f64(X, self.device)
        ys = [_dev_f64(y, self.device).reshape(-1) for y in ys]
        n, d = X.shape
        k = len(ys)
        if any(y.shape[0] != n for y in ys):
            raise ValueError("gp_lml_grad_batch: every y needs one value per input row")
        ls = np.ascontiguousarray(np.broadcast_to(np.asarray(lengthscales, np.float64), (k, d)))
        var = np.ascontiguousarray(np.asarray(variances, np.float64).reshape(k))
        kid = _KERNEL_IDS[kernel]
        yptr = (ctypes.c_void_p * k)(*[y.data_ptr() for y in ys])
        lml = np.zeros(k)
        grad = np.zeros((k, d + 2 if noise_grad else d + 1))
        jit = np.zeros(k)
        status = np.zeros(k, np.int32)
        dp = ctypes.POINTER(ctypes.c_double)
        self._stream()
        if noise_grad:
            nz = np.ascontiguousarray(np.broadcast_to(np.asarray(noise, np.float64), (k,)))
            self._check(self.lib.omb_gp_lml_grad_noise_batch(
                self._h, kid, k, n, d, _ptr(X), ctypes.cast(yptr, ctypes.c_void_p), ls.ctypes.data_as(dp),
                var.ctypes.data_as(dp), nz.ctypes.data_as(dp), lml.ctypes.data_as(dp), grad.ctypes.data_as(dp),
                jit.ctypes.data_as(dp), ctypes.c_void_p(status.ctypes.data)), "omb_gp_lml_grad_noise_batch")
            return lml, grad, jit, status
        self._check(self.lib.omb_gp_lml_grad_batch(
            self._h, kid, k, n, d, _ptr(X), ctypes.cast(yptr, ctypes.c_void_p), ls.ctypes.data_as(dp),
            var.ctypes.data_as(dp), float(noise), lml.ctypes.data_as(dp), grad.ctypes.data_as(dp),
            jit.ctypes.data_as(dp), ctypes.c_void_p(status.ctypes.data)), "omb_gp_lml_grad_batch")
        return lml, grad, jit, status

    def gp_fit_state(self, obj, X, y, lengthscale, variance, noise=0.0, kernel="matern52"):
        """Factorise on the device and install objective ``obj`` (omb_gp_fit_state); returns the jitter."""
        X = _dev_f64(X, self.device)
        y = _dev_f64(y, self.device).reshape(-1)
        n, d = X.shape
        ls = np.broadcast_to(np.asarray(lengthscale, np.float64), (d,))
        kid = _KERNEL_IDS[kernel]
        jit = ctypes.c_double()
        self._stream()
        self._check(self.lib.omb_gp_fit_state(self._h, int(obj), kid, n, d, _ptr(X), _ptr(y), _lib.darr(ls),
                                              float(variance), float(noise), ctypes.byref(jit)), "omb_gp_fit_state")
        self._gp_keep[obj] = (X, y)
        self.gp_info[obj] = dict(n=n, d=d, variance=float(variance), kernel=kernel)
        return jit.value

    def gp_append(self, obj, Xnew, ynew=None, noise=0.0):
        """Condition objective ``obj``'s installed state on the rows of Xnew (q, d), one after another, without a
        refit (omb_gp_append).  ``ynew`` (q,) are their observed values; None is the Kriging believer: each point
        takes the posterior mean it has when it is appended, so the mean surface stays and only σ² shrinks.
        ``noise``: the σ_n² the state was factorised with (plus jitchol's jitter, where known).  Returns
        (mu (q,), delta2 (q,)) as numpy: every point's predictive mean and δ² = σ² + σ_n² + 1e-8 at its turn.
        OMBError (OMB_ENOTPD) for a δ² ≤ 0, the installed state then being what it was."""
        Xnew = _dev_f64(Xnew, self.device)
        if Xnew.dim() == 1:
            Xnew = Xnew.reshape(1, -1)
        self._check_width(Xnew, obj)
        q = Xnew.shape[0]
        y = None
        if ynew is not None:
            y = _dev_f64(ynew, self.device).reshape(-1)
            if y.shape[0] != q:
                raise ValueError(f"gp_append: {y.shape[0]} values for {q} points")
        mu = torch.empty(max(q, 1), dtype=torch.float64, device=self.device)
        d2 = torch.empty_like(mu)
        self._stream()
        self._check(self.lib.omb_gp_append(self._h, int(obj), q, _ptr(Xnew), _ptr(y) if y is not None else None,
                                           float(noise), _ptr(mu), _ptr(d2)), "omb_gp_append")
        self.gp_info[obj]["n"] += q
        return mu[:q].cpu().numpy(), d2[:q].cpu().numpy()

    # ------------------------------------------------------------------ Thompson sampling (TuRBO)
    def posterior_cov(self, obj, Xc, out=None):
        """μ (N,), Σ (N, N): GPy predict(Xc, full_cov=True) of objective ``obj`` (σ_n² = 0)."""
        Xc = _dev_f64(Xc, self.device)
        self._check_width(Xc, obj)
        N = Xc.shape[0]
        mu, cov = out if out is not None else (self._out(None, N), self._out(None, (N, N)))
        self._stream()
        self._check(self.lib.omb_posterior_cov(self._h, int(obj), _ptr(Xc), N, _ptr(mu), _ptr(cov)),
                    "omb_posterior_cov")
        return mu, cov

    def cholesky(self, A, jitter=0.0):
        """In place: lower triangle of A (N, N) ← chol(A + jitter·I); returns LAPACK's info (0 = ok)."""
        if A.dtype != torch.float64 or A.dim() != 2 or A.shape[0] != A.shape[1] or A.stride(1) != 1:
            raise ValueError("cholesky: A must be a square fp64 device matrix with unit column stride")
        info = ctypes.c_int()
        self._stream()
        self._check(self.lib.omb_cholesky(self._h, _ptr(A), A.shape[0], A.stride(0), float(jitter), ctypes.byref(info)),
                    "omb_cholesky")
        return info.value

    def posterior_samples(self, obj, Xc, Zt, jitter_rel=1e-10, max_tries=8, out=None):
        """Y (B, N): B joint posterior samples μ + chol(Σ + jI) z_b at Xc, z_b = row b of Zt (B, N).

        Returns (Y, j) with j the absolute jitter that made Σ + jI factorisable."""
        Xc = _dev_f64(Xc, self.device)
        self._check_width(Xc, obj)
        Zt = _dev_f64(Zt, self.device)
        N = Xc.shape[0]
        B = Zt.shape[0]
        if Zt.dim() != 2 or Zt.shape[1] != N:
            raise ValueError(f"Zt must be (B, {N}), got {tuple(Zt.shape)}")
        Y = self._out(out, (B, N))
        used = ctypes.c_double()
        self._stream()
        self._check(self.lib.omb_posterior_samples(self._h, int(obj), _ptr(Xc), N, _ptr(Zt), B, float(jitter_rel),
                                                   int(max_tries), _ptr(Y), ctypes.byref(used)),
                    "omb_posterior_samples")
        return Y, used.value

    def thompson_select(self, Y, out=None):
        """TuRBO's greedy per-sample arg-min over Y (B, N) → indices (B,) int64 (device)."""
        Y = _dev_f64(Y, self.device)
        B, N = Y.shape
        idx = self._out(out, B, torch.int64)
        self._stream()
        self._check(self.lib.omb_thompson_select(self._h, _ptr(Y), B, N, _ptr(idx)), "omb_thompson_select")
        return idx

    # ------------------------------------------------------------------ posterior sample paths
    def paths_set(self, obj, omega, phase, w, z=None, noise=0.0):
        """Install S posterior sample paths of objective ``obj`` (omb_paths_set): frequencies omega (m, d) of x/ℓ,
        phases (m,), standard normals w (m, S) and z (n_train, S) (None: ε = 0), ``noise`` the σ_n² the state was
        factorised with.  Host arrays (optimobo_amd.paths.draw_path_inputs draws them); the paths stand until the
        objective's state changes."""
        omega = np.ascontiguousarray(omega, dtype=np.float64)
        phase = np.ascontiguousarray(phase, dtype=np.float64).reshape(-1)
        w = np.ascontiguousarray(w, dtype=np.float64)
        info = self.gp_info.get(obj)
        if omega.ndim != 2 or w.ndim != 2 or phase.shape[0] != omega.shape[0] or w.shape[0] != omega.shape[0]:
            raise ValueError(f"paths_set: shapes omega{omega.shape} phase{phase.shape} w{w.shape}")
        m, S = w.shape
        if info is not None and omega.shape[1] != info["d"]:
            raise ValueError(f"paths_set: omega has {omega.shape[1]} columns but objective {obj}'s GP has "
                             f"n_var={info['d']}")
        if z is not None:
            z = np.ascontiguousarray(z, dtype=np.float64)
            if info is not None and z.shape != (info["n"], S):
                raise ValueError(f"paths_set: z{z.shape} is not (n_train, S) = ({info['n']}, {S})")
        self._stream()
        self._paths_S.pop(obj, None)
        self._check(self.lib.omb_paths_set(self._h, int(obj), S, m, _lib.host_ptr(omega), _lib.host_ptr(phase),
                                           _lib.host_ptr(w), _lib.host_ptr(z) if z is not None else None,
                                           float(noise)), "omb_paths_set")
        self._paths_S[obj] = S

    def paths_eval(self, Xc, n_obj=None, out=None):
        """The installed paths of objectives 0..n_obj-1 at candidates Xc (N, d) → (n_obj, S, N) (omb_paths_eval).
        ``out``: a (n_obj, S, ld ≥ N) tensor whose rows are contiguous; columns past N stay untouched."""
        Xc = _dev_f64(Xc, self.device)
        self._check_width(Xc)
        n_obj = n_obj if n_obj is not None else len(self.gp_info)
        N = Xc.shape[0]
        if out is None:
            out = self._out(None, (n_obj, self._paths_S.get(0, 1), N))
        else:
            # the kernel writes row (o·S + s) at pitch ld: any other layout would be written out of bounds
            S = self._paths_S.get(0)
            if S is None or not isinstance(out, torch.Tensor) or out.dtype != torch.float64 \
                    or out.device != self.device or out.dim() != 3 or tuple(out.shape[:2]) != (n_obj, S) \
                    or out.shape[2] < N or (out.shape[2] > 1 and out.stride(2) != 1) \
                    or out.stride(0) != S * out.stride(1) or out.stride(1) < N:
                raise ValueError(f"paths_eval: out must be a ({n_obj}, S, ld >= {N}) fp64 tensor on {self.device} with "
                                 "unit column stride and evenly pitched rows, S the paths installed on objective 0")
        ld = out.stride(1)
        self._stream()
        self._check(self.lib.omb_paths_eval(self._h, int(n_obj), _ptr(Xc), N, int(ld), _ptr(out)), "omb_paths_eval")
        return out

    def paths_grad(self, Xc, n_obj=None, ld=None):
        """The installed paths of objectives 0..n_obj-1 and their gradients at candidates Xc (N, d) (omb_paths_grad):
        (vals (n_obj, S, N), bitwise ``paths_eval``'s; grad (n_obj, S, d, N), grad[o, s, j, i] = ∂f_{o,s}/∂x_j at
        Xc[i]).  ``ld`` ≥ N pitches the rows of both (views of the first N columns are returned)."""
        Xc = _dev_f64(Xc, self.device)
        self._check_width(Xc)
        n_obj = n_obj if n_obj is not None else len(self.gp_info)
        N, d = Xc.shape
        ld = N if ld is None else int(ld)
        if ld < N:
            raise ValueError(f"paths_grad: ld={ld} < N={N}")
        S = self._paths_S.get(0, 1)
        vals = torch.empty((n_obj, S, ld), dtype=torch.float64, device=self.device)
        grad = torch.empty((n_obj, S, d, ld), dtype=torch.float64, device=self.device)
        self._stream()
        self._check(self.lib.omb_paths_grad(self._h, int(n_obj), _ptr(Xc), N, ld, _ptr(vals), _ptr(grad)),
                    "omb_paths_grad")
        return vals[:, :, :N], grad[:, :, :, :N]

    def hvi_paths_grad(self, y, dy, coords, box_off, boxes, per_path=False):
        """omb_hvi_paths_grad: ``hvi_paths``' value and its gradient through the paths — y (k, S, N) and dy
        (k, S, d, N) as ``paths_grad`` returns them (the same pitch) → (v (N,), g (N, d)); with ``per_path`` also
        (t (S, N), tg (S, N, d)), the per-path improvement t_s and ∂t_s/∂x.  The (N, d) results are transposed views
        of the device layout."""
        c, o, b = self._box_lists_host(coords, box_off, boxes, "hvi_paths_grad")
        S, k, C = c.shape
        if not isinstance(y, torch.Tensor) or y.dtype != torch.float64 or y.device != self.device or y.dim() != 3 \
                or tuple(y.shape[:2]) != (k, S) or (y.shape[2] > 1 and y.stride(2) != 1) \
                or y.stride(0) != S * y.stride(1) or y.stride(1) < y.shape[2]:
            raise ValueError(f"hvi_paths_grad: y must be a ({k}, {S}, N) fp64 tensor on {self.device} with unit "
                             "column stride and evenly pitched rows")
        N, ld = y.shape[2], y.stride(1)
        if not isinstance(dy, torch.Tensor) or dy.dtype != torch.float64 or dy.device != self.device \
                or dy.dim() != 4 or tuple(dy.shape[:2]) != (k, S) or dy.shape[3] != N or dy.shape[2] < 1 \
                or (N > 1 and dy.stride(3) != 1) or dy.stride(2) != ld or dy.stride(1) != dy.shape[2] * ld \
                or dy.stride(0) != S * dy.stride(1):
            raise ValueError(f"hvi_paths_grad: dy must be a ({k}, {S}, d, {N}) fp64 tensor on {self.device} at y's "
                             f"pitch {ld}")
        d = dy.shape[2]
        out = torch.empty(N, dtype=torch.float64, device=self.device)
        grad = torch.empty((d, ld), dtype=torch.float64, device=self.device)
        t = torch.empty((S, ld), dtype=torch.float64, device=self.device) if per_path else None
        tg = torch.empty((S, d, ld), dtype=torch.float64, device=self.device) if per_path else None
        cd = torch.as_tensor(c, device=self.device)
        bd = self._boxes_dev(b)
        self._stream()
        self._check(self.lib.omb_hvi_paths_grad(self._h, k, S, d, _ptr(y), _ptr(dy), ld, N, _ptr(cd), C,
                                                _lib.host_ptr(o), _ptr(bd), _ptr(out), _ptr(grad),
                                                _ptr(t) if per_path else None, _ptr(tg) if per_path else None),
                    "omb_hvi_paths_grad")
        if per_path:
            return out, grad[:, :N].T, t[:, :N], tg[:, :, :N].permute(0, 2, 1)
        return out, grad[:, :N].T

    def paths_min(self, Xc, n_obj=None, offset=0):
        """The minimum of every installed path of objectives 0..n_obj-1 over candidates Xc (N, d) (omb_paths_min):
        (values (n_obj, S) fp64, indices (n_obj, S) int64 = the lowest arg-min + offset), bitwise
        ``paths_eval(Xc).min(-1)`` without the (n_obj, S, N) matrix.  NaN never wins; an empty batch or an all-NaN
        row gives (+inf, −1)."""
        Xc = _dev_f64(Xc, self.device)
        if Xc.shape[0]:
            self._check_width(Xc)
        n_obj = n_obj if n_obj is not None else len(self.gp_info)
        res = torch.empty((max(1, int(n_obj)), 16, 2), dtype=torch.float64, device=self.device)   # S ≤ 16
        self._stream()
        self._check(self.lib.omb_paths_min(self._h, int(n_obj), _ptr(Xc), Xc.shape[0], int(offset), _ptr(res)),
                    "omb_paths_min")
        S = self._paths_S[0]
        res = res.reshape(-1)[:2 * n_obj * S].reshape(n_obj, S, 2)
        return res[:, :, 0].contiguous(), res[:, :, 1].to(torch.int64)

    def ea_search(self, pop, tape, best, lower, upper, mode=0, var_eps=1e-6):
        """ParEGO (mode 0: EI of objective 0) / KEEP (mode 1: μ of objective 1 · EI of objective 0)
        evolutionary acquisition search (omb_ea_search) from the temporary population `pop` (P, d) and
        a tape of the reference's random draws (optimobo_amd.ea.ea_tape) → (best x (d,), best fitness),
        host numpy.  Synchronises."""
        pop = np.ascontiguousarray(pop, np.float64)
        P, d = pop.shape
        if tape.beta.shape[1:] != (d,) or tape.mut.shape[1:] != (d,) or tape.sel.shape[1:] != (4,):
            raise ValueError("tape does not match the population width")
        sel = tape.sel
        if len(sel) and (sel[:, :2].min() < 1 or sel[:, :2].max() > P - 1 or sel[:, 2:].min() < 1
                         or sel[:, 2:].max() > P - 2):
            raise ValueError("tournament samples outside range(1, P) / range(1, P - 1)")
        dv = self.device
        t_pop = torch.as_tensor(pop, device=dv)
        self._check_width(t_pop)
        if mode == _lib.EA_PARETO_EI:
            self._check_width(t_pop, 1)
        t_sel = torch.as_tensor(np.ascontiguousarray(sel, np.int32), device=dv)
        t_cross = torch.as_tensor(np.ascontiguousarray(tape.cross, np.int8), device=dv)
        t_beta = torch.as_tensor(np.ascontiguousarray(tape.beta, np.float64), device=dv)
        t_mut = torch.as_tensor(np.ascontiguousarray(tape.mut, np.int8), device=dv)
        t_lo = torch.as_tensor(np.ascontiguousarray(lower, np.float64).reshape(d), device=dv)
        t_hi = torch.as_tensor(np.ascontiguousarray(upper, np.float64).reshape(d), device=dv)
        out = torch.empty(d + 1, dtype=torch.float64, device=dv)
        self._stream()
        self._check(self.lib.omb_ea_search(self._h, int(mode), float(best), float(var_eps), _ptr(t_pop), P,
                                           int(tape.iters), _ptr(t_sel), _ptr(t_cross), _ptr(t_beta), _ptr(t_mut),
                                           _ptr(t_lo), _ptr(t_hi), _ptr(out)), "omb_ea_search")
        o = out.cpu().numpy()
        return o[:d].copy(), float(o[d])

    def timing(self, level=2):
        """0 off, 1 posterior only, 2 every stage of the fused chain (see omb_timing)."""
        self._stream()
        self._check(self.lib.omb_timing(self._h, int(level)), "omb_timing")

    def timing_read(self):
        """{stage: summed ms} over the fused chains since the last read, and their count."""
        ms = (ctypes.c_double * 4)()
        n = ctypes.c_int64()
        self._stream()
        self._check(self.lib.omb_timing_read(self._h, ms, ctypes.byref(n)), "omb_timing_read")
        return dict(zip(("sobol", "posterior", "acquisition", "argmax"), list(ms))), n.value
