"""The order of every acquisition entry point's argument checks, pinned by calls that carry two faults whose codes
(or messages) differ: the one reported names the check that runs first.  Every call but the last test's omb_eval is
rejected before any device access, so non-null device pointers are the fake aligned address 8."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from optimobo_amd import _lib  # noqa: E402

P8 = ctypes.c_void_p(8)
N = 4
R2 = _lib.darr([1.0, 1.0])
R3 = _lib.darr([1.0, 1.0, 1.0])


@pytest.fixture()
def ctx():
    from optimobo_amd.device import AcqContext
    c = AcqContext(0)
    yield c
    c.close()


def _err(ctx):
    return ctx.lib.omb_last_error(ctx._h).decode()


def test_ehvi2d_checks_moments_then_geometry_then_front_size(ctx):
    lib, h = ctx.lib, ctx._h
    # a null front and P = 0: the stand-alone entry meets the null front first, the plan entry the size
    assert lib.omb_ehvi2d(h, P8, P8, N, N, None, 0, R2, 1.0, 0.1, _lib.EHVI_REFERENCE, P8) == _lib.OMB_EINVAL
    assert lib.omb_plan_ehvi2d(h, None, 0, R2, 1.0, 0.1, _lib.EHVI_REFERENCE) == _lib.OMB_EUNSUP
    # N < 0 (check_moments) before P = 0 (check_ehvi2d)
    assert lib.omb_ehvi2d(h, P8, P8, N, -1, P8, 0, R2, 1.0, 0.1, _lib.EHVI_REFERENCE, P8) == _lib.OMB_EINVAL


def test_hvpoi_checks_moments_then_geometry_then_cell_count(ctx):
    lib, h = ctx.lib, ctx._h
    assert lib.omb_hvpoi(h, P8, P8, N, N, None, 0, P8) == _lib.OMB_EINVAL
    assert lib.omb_plan_hvpoi(h, None, 0) == _lib.OMB_EUNSUP


def test_own_check_before_moments(ctx):
    """omb_ehvi_mc, omb_ehvi_boxes, omb_ehvi_boxes_k, omb_ei_ext and omb_expdec validate their own scalars first."""
    lib, h = ctx.lib, ctx._h
    assert lib.omb_ehvi_mc(h, 3, P8, P8, N, -1, P8, 0, R3, 0.0, P8, P8) == _lib.OMB_EUNSUP        # M = 0, N = -1
    assert lib.omb_ehvi_boxes(h, 4, P8, P8, N, -1, P8, 4, P8, 1, P8) == _lib.OMB_EUNSUP           # k = 4, N = -1
    assert lib.omb_ehvi_boxes(h, 3, P8, P8, N, N, P8, 1, P8, 0, P8) == _lib.OMB_EUNSUP            # C = 1, B = 0
    assert lib.omb_ehvi_boxes_k(h, 4, None, P8, N, N, P8, 1, P8, 1, P8) == _lib.OMB_EUNSUP        # C = 1, mu = NULL
    # a null grid before the box list's alignment (both OMB_EINVAL: the message tells them apart)
    assert lib.omb_ehvi_boxes_k(h, 4, P8, P8, N, N, None, 2, ctypes.c_void_p(6), 1, P8) == _lib.OMB_EINVAL
    assert "null grid/box list" in _err(ctx)
    assert lib.omb_ehvi_boxes_k(h, 4, P8, P8, N, N, P8, 2, ctypes.c_void_p(6), 1, P8) == _lib.OMB_EINVAL
    assert "not 4-byte aligned" in _err(ctx)
    assert lib.omb_ei_ext(h, _lib.EI_PLAIN, 2, P8, P8, N, -1, 0.0, 0.0, 0.0, P8) == _lib.OMB_EINVAL
    assert "kind" in _err(ctx) and "N=" not in _err(ctx)
    # scalarisation 99 does not exist, N = -1: build_scal answers
    w = _lib.darr([0.5, 0.5])
    assert lib.omb_expdec(h, 2, P8, P8, N, -1, P8, 8, 99, None, w, w, w, 0.0, P8) == _lib.OMB_EINVAL
    assert _err(ctx) == "unknown scalarisation 99"


def test_failed_plan_leaves_no_plan(ctx):
    lib, h = ctx.lib, ctx._h
    ctx.plan_ei(0.5)
    coords = np.ascontiguousarray(np.tile(np.linspace(0.0, 1.0, 3), (4, 1)))      # k = 4, C = 3
    boxes = np.ascontiguousarray(np.tile([0, 3], 4).reshape(1, 8), dtype=np.uint16)   # hi = 3 >= C
    rc = lib.omb_plan_ehvi_boxes_k(h, 4, _lib.host_ptr(coords), 3, _lib.host_ptr(boxes), 1)
    assert rc == _lib.OMB_EINVAL and "grid indices" in _err(ctx)
    assert lib.omb_eval(h, P8, N, P8) == _lib.OMB_ESTATE


def test_failed_constraints_leave_the_plan(ctx):
    from optimobo_amd.gp import GPState
    lib, h = ctx.lib, ctx._h
    rng = np.random.default_rng(0)
    X = rng.uniform(0, 1, (10, 2))
    y = np.sin(3 * X).sum(1)
    ctx.set_gp_state(0, GPState(X, y, [0.5, 0.5], 1.0))
    ctx.plan_ei(float(y.min()))
    Xc = torch.as_tensor(rng.uniform(0, 1, (3, 2)), device="cuda:0")
    before = ctx.eval(Xc)
    assert lib.omb_plan_constraints(h, -1, 1e-5) == _lib.OMB_EINVAL
    after = ctx.eval(Xc)
    assert after.shape == (3,) and torch.equal(before, after)
