"""CPU-only: csrc/trust_region.h, the one statement of DESIGN.md 12's trust-region rulings that the four Levenberg-Marquardt
solvers run on the device, compiled for the host (libdsm_trust_region.so) and held to the formulas of DESIGN.md 12 written out
here in Python floats.  Both sides are the same IEEE double operations in the same order, so every assertion is an equality."""
import ctypes
import math
import os
import sys

import pytest

ACCEPTED, REJECTED, INVALID, TOLERANCE = 1, 2, 3, 4  # as dsm_refine_absolute_poses documents steps_out
CONVERGENCE, NO_CONVERGENCE, FAILURE = 0, 1, 2         # DSM_BA_*
INF, NAN = math.inf, math.nan
DBL_MIN = sys.float_info.min


class Options(ctypes.Structure):
    _fields_ = [(n, ctypes.c_double) for n in ("ftol", "gtol", "ptol", "min_relative_decrease", "max_radius", "min_radius")] + \
               [(n, ctypes.c_int) for n in ("max_iterations", "max_consecutive_invalid_steps")]


class State(ctypes.Structure):
    _fields_ = [(n, ctypes.c_double) for n in ("cost", "radius", "dec", "last_rho", "gnorm", "m_accept", "m_grad", "m_func", "m_param")] + \
               [(n, ctypes.c_int) for n in ("iter", "n_succ", "n_rej", "n_invalid", "n_invalid_total", "accepted", "term", "done")]


@pytest.fixture(scope="module")
def lib():
    from dagsfm_amd import capi
    path = os.path.join(os.path.dirname(capi.LIB_PATH), "libdsm_trust_region.so")
    assert os.path.exists(path), "build first: " + path
    L = ctypes.CDLL(path)
    L.dsm_tr_init.argtypes = [ctypes.POINTER(State), ctypes.c_double]
    L.dsm_tr_init.restype = None
    L.dsm_tr_ceres_defaults.argtypes = [ctypes.POINTER(Options)]
    L.dsm_tr_ceres_defaults.restype = None
    L.dsm_tr_margin.argtypes = [ctypes.c_double, ctypes.c_double]
    L.dsm_tr_margin.restype = ctypes.c_double
    L.dsm_tr_decide.argtypes = [ctypes.POINTER(State), ctypes.POINTER(Options), ctypes.c_int] + [ctypes.c_double] * 4
    L.dsm_tr_decide.restype = ctypes.c_int
    L.dsm_tr_end_iteration.argtypes = [ctypes.POINTER(State), ctypes.POINTER(Options), ctypes.c_int]
    L.dsm_tr_end_iteration.restype = None
    assert L.dsm_tr_sizeof_state() == ctypes.sizeof(State) and L.dsm_tr_sizeof_options() == ctypes.sizeof(Options)
    return L


def start(lib, cost=1.0, radius=1e4, **opt):
    """A state at iteration 0 with the given cost, and ceres' default options with both step tolerances off unless given."""
    o, s = Options(), State()
    lib.dsm_tr_ceres_defaults(o)
    o.ftol = o.ptol = 0.0
    for k, v in opt.items():
        setattr(o, k, v)
    lib.dsm_tr_init(s, radius)
    s.cost = cost
    return s, o


def decide(lib, s, o, cand, mcc=1.0, step2=1.0, x2=1.0, solved=True):
    return lib.dsm_tr_decide(s, o, int(solved), cand, mcc, step2, x2)


def margin(a, thr):
    """DESIGN.md 12, **Margins**: |a - thr| / max(|a|, |thr|)"""
    den = max(abs(a), abs(thr))
    return abs(a - thr) / den if den > 0.0 else 0.0


def test_defaults_and_initial_state(lib):
    s, o = State(), Options()
    lib.dsm_tr_ceres_defaults(o)
    assert (o.ftol, o.gtol, o.ptol, o.min_relative_decrease, o.max_radius, o.min_radius) == (1e-6, 1e-10, 1e-8, 1e-3, 1e16, 1e-32)
    assert (o.max_iterations, o.max_consecutive_invalid_steps) == (50, 5)
    lib.dsm_tr_init(s, 1e4)
    assert (s.cost, s.radius, s.dec, s.gnorm) == (0.0, 1e4, 2.0, 0.0) and math.isnan(s.last_rho)
    assert (s.m_accept, s.m_grad, s.m_func, s.m_param) == (INF,) * 4
    assert (s.iter, s.n_succ, s.n_rej, s.n_invalid, s.n_invalid_total, s.accepted, s.term, s.done) == (0,) * 8


def test_step_codes(lib):
    s, o = start(lib, cost=1.0, ptol=2.0 ** -10)
    assert decide(lib, s, o, 0.5) == ACCEPTED == 1          # rho = 0.5
    assert decide(lib, s, o, 0.6) == REJECTED == 2          # the cost goes up
    assert decide(lib, s, o, 0.4, solved=False) == INVALID == 3
    assert decide(lib, s, o, 0.4, step2=0.0) == TOLERANCE == 4
    assert (s.iter, s.n_succ, s.n_rej, s.n_invalid_total, s.done, s.term) == (4, 1, 1, 1, 1, CONVERGENCE)


def test_invalid_steps_shrink_the_radius_and_fail_at_the_cap(lib):
    s, o = start(lib, max_consecutive_invalid_steps=4)
    radius, factor = 1e4, 2.0
    for k in range(1, 4):  # / 2, / 4, / 8
        assert decide(lib, s, o, 0.5, solved=False) == INVALID
        radius, factor = radius / factor, factor * 2.0
        assert (s.radius, s.dec, s.n_invalid, s.n_invalid_total, s.iter, s.done) == (radius, factor, k, k, k, 0)
        assert s.accepted == 0 and s.cost == 1.0 and math.isnan(s.last_rho)
    assert radius == 1e4 / 2.0 / 4.0 / 8.0
    assert decide(lib, s, o, 0.5, solved=False) == INVALID
    assert (s.term, s.done, s.n_invalid, s.n_invalid_total, s.iter) == (FAILURE, 1, 4, 4, 4)
    assert (s.radius, s.dec) == (radius, factor)  # the failing step leaves the radius alone


def test_a_valid_step_resets_the_consecutive_count_only(lib):
    s, o = start(lib, max_consecutive_invalid_steps=3)
    for _ in range(2):
        assert decide(lib, s, o, 0.5, solved=False) == INVALID
    assert decide(lib, s, o, 2.0) == REJECTED  # valid, not accepted
    assert (s.n_invalid, s.n_invalid_total, s.done) == (0, 2, 0)
    for k in (1, 2):
        assert decide(lib, s, o, 0.5, solved=False) == INVALID
        assert (s.n_invalid, s.n_invalid_total, s.done) == (k, 2 + k, 0)
    assert decide(lib, s, o, 0.5) == ACCEPTED
    assert (s.n_invalid, s.n_invalid_total) == (0, 4)
    for k in (1, 2, 3):
        assert decide(lib, s, o, 0.25, solved=False) == INVALID
    assert (s.term, s.done, s.n_invalid, s.n_invalid_total) == (FAILURE, 1, 3, 7)


@pytest.mark.parametrize("kw", [dict(cand=INF), dict(cand=-INF), dict(cand=NAN), dict(cand=0.5, mcc=0.0), dict(cand=0.5, mcc=-1.0),
                                dict(cand=0.5, mcc=NAN), dict(cand=0.5, mcc=INF), dict(cand=0.5, step2=INF), dict(cand=0.5, step2=NAN)])
def test_what_counts_as_invalid(lib, kw):
    """A non-finite candidate cost, model_cost_change <= 0 or non-finite, |delta| non-finite: invalid although the solve succeeded"""
    s, o = start(lib)
    assert decide(lib, s, o, **kw) == INVALID
    assert (s.n_invalid, s.radius, s.dec, s.cost, s.accepted) == (1, 1e4 / 2.0, 4.0, 1.0, 0)
    assert (s.m_accept, s.m_func, s.m_param) == (INF, INF, INF)  # no test was reached


def test_parameter_tolerance_comes_before_function_tolerance(lib):
    ptol, ftol = 2.0 ** -10, 2.0 ** -4
    x2 = 9.0
    thr = ptol * (math.sqrt(x2) + ptol)
    # both tolerances hold: only the parameter test is reached
    s, o = start(lib, cost=1.0, ptol=ptol, ftol=ftol)
    assert decide(lib, s, o, 1.0 - 2.0 ** -6, step2=thr * thr, x2=x2) == TOLERANCE  # |delta| = thr exactly: <=
    assert math.sqrt(thr * thr) == thr
    assert (s.term, s.done, s.accepted, s.cost, s.iter, s.n_succ) == (CONVERGENCE, 1, 0, 1.0, 1, 0)
    assert (s.m_param, s.m_func, s.m_accept) == (0.0, INF, INF)
    assert (s.radius, s.dec) == (1e4, 2.0)
    # one ulp above the parameter threshold: the function test decides, the step is still not applied
    s, o = start(lib, cost=1.0, ptol=ptol, ftol=ftol)
    up = math.nextafter(thr, INF)
    step2 = up * up
    assert math.sqrt(step2) > thr
    cand = 1.0 - 2.0 ** -4  # |change| = ftol * cost exactly: <=
    assert decide(lib, s, o, cand, step2=step2, x2=x2) == TOLERANCE
    assert (s.term, s.done, s.accepted, s.cost, s.n_succ) == (CONVERGENCE, 1, 0, 1.0, 0)
    assert s.m_param == margin(math.sqrt(step2), thr) and s.m_func == margin(abs(1.0 - cand), ftol * 1.0) == 0.0
    assert s.m_accept == INF and math.isnan(s.last_rho)
    # neither holds: the step is judged by rho
    s, o = start(lib, cost=1.0, ptol=ptol, ftol=ftol)
    assert decide(lib, s, o, 0.5, step2=step2, x2=x2) == ACCEPTED
    assert s.m_func == margin(0.5, ftol) and s.done == 0


def test_rho_at_the_threshold_rejects_and_one_ulp_above_accepts(lib):
    mrd = 1e-3
    cost = 2e-3
    # rho = (cost - candidate) / model_cost_change with model_cost_change = 1: the change is rho
    cand = 1e-3
    assert (cost - cand) / 1.0 == mrd
    s, o = start(lib, cost=cost)
    assert decide(lib, s, o, cand) == REJECTED
    assert (s.last_rho, s.accepted, s.cost, s.n_rej, s.n_succ) == (mrd, 0, cost, 1, 0)
    assert (s.radius, s.dec) == (1e4 / 2.0, 4.0)
    assert s.m_accept == abs((cost - cand) - mrd * 1.0) / max(cost, DBL_MIN) == 0.0
    cand = math.nextafter(1e-3, 0.0)
    rho = (cost - cand) / 1.0
    assert rho == math.nextafter(mrd, INF)
    s, o = start(lib, cost=cost)
    assert decide(lib, s, o, cand) == ACCEPTED
    tmp = 2.0 * rho - 1.0
    assert (s.last_rho, s.accepted, s.cost, s.n_rej, s.n_succ) == (rho, 1, cand, 0, 1)
    assert (s.radius, s.dec) == (min(1e16, 1e4 / max(1.0 / 3.0, 1.0 - tmp * tmp * tmp)), 2.0)
    assert s.m_accept == abs((cost - cand) - mrd * 1.0) / max(cost, DBL_MIN) > 0.0


@pytest.mark.parametrize("cand,mcc", [(0.0, 1.0), (0.5, 1.0), (0.75, 1.0), (0.25, 3.0), (0.9, 0.125), (0.3, 0.7000000000000001)])
def test_radius_after_an_accepted_step(lib, cand, mcc):
    s, o = start(lib, cost=1.0, radius=37.5)
    for _ in range(2):  # two rejections first: the factor is 8 when the step is accepted
        assert decide(lib, s, o, 1.5, mcc=mcc) == REJECTED
    radius = 37.5 / 2.0 / 4.0
    assert (s.radius, s.dec) == (radius, 8.0)
    assert decide(lib, s, o, cand, mcc=mcc) == ACCEPTED
    rho = (1.0 - cand) / mcc
    tmp = 2.0 * rho - 1.0
    assert s.radius == min(1e16, radius / max(1.0 / 3.0, 1.0 - tmp * tmp * tmp))
    assert (s.dec, s.cost, s.last_rho, s.accepted, s.n_succ, s.n_rej) == (2.0, cand, rho, 1, 1, 2)
    assert s.m_accept == min(abs((1.0 - 1.5) - 1e-3 * mcc) / 1.0, abs((1.0 - cand) - 1e-3 * mcc) / 1.0)


def test_radius_is_clamped_and_rejections_divide_by_a_doubling_factor(lib):
    s, o = start(lib, cost=1.0, radius=9e15)
    assert decide(lib, s, o, 0.0) == ACCEPTED  # rho = 1: the radius would triple
    assert 9e15 / max(1.0 / 3.0, 1.0 - 1.0) > 1e16 and s.radius == 1e16
    s, o = start(lib, cost=1.0, radius=9e15, max_radius=1e300)
    assert decide(lib, s, o, 0.0) == ACCEPTED
    assert s.radius == 9e15 / (1.0 / 3.0)
    s, o = start(lib, cost=1.0, radius=3.0)
    radius, factor = 3.0, 2.0
    for k in range(1, 6):
        assert decide(lib, s, o, 1.0 + k) == REJECTED  # rho < 0
        radius, factor = radius / factor, factor * 2.0
        assert (s.radius, s.dec, s.n_rej, s.cost, s.last_rho) == (radius, factor, k, 1.0, (1.0 - (1.0 + k)) / 1.0)
    assert factor == 64.0


def test_end_of_iteration_order(lib):
    end = lib.dsm_tr_end_iteration
    # the cap comes first, even where the gradient test would pass and the radius is below its minimum
    s, o = start(lib, max_iterations=1, gtol=1.0)
    assert decide(lib, s, o, 0.5) == ACCEPTED
    s.gnorm, s.radius = 0.5, 1e-40
    end(s, o, 1)
    assert (s.term, s.done, s.m_grad) == (NO_CONVERGENCE, 1, INF)
    # the gradient test runs only on a fresh gradient
    s, o = start(lib, gtol=1.0)
    s.gnorm = 0.5
    end(s, o, 0)
    assert (s.done, s.m_grad) == (0, INF)
    end(s, o, 1)
    assert (s.term, s.done, s.m_grad) == (CONVERGENCE, 1, margin(0.5, 1.0))
    s, o = start(lib, gtol=1.0)
    s.gnorm = 1.0  # at the tolerance: <=
    end(s, o, 1)
    assert (s.term, s.done, s.m_grad) == (CONVERGENCE, 1, 0.0)
    # the minimum radius is tested last: the gradient margin of that call is recorded, a radius at the minimum goes on
    s, o = start(lib, gtol=1.0)
    s.gnorm, s.radius = 2.0, 1e-32
    end(s, o, 1)
    assert (s.done, s.m_grad) == (0, margin(2.0, 1.0))
    s.radius = math.nextafter(1e-32, 0.0)
    end(s, o, 0)
    assert (s.term, s.done) == (CONVERGENCE, 1)
    # max_iterations = 0 ends at iteration 0
    s, o = start(lib, max_iterations=0, gtol=1.0)
    s.gnorm = 0.5
    end(s, o, 1)
    assert (s.term, s.done, s.iter, s.m_grad) == (NO_CONVERGENCE, 1, 0, INF)
    # a finished loop stays as it ended
    s, o = start(lib, max_consecutive_invalid_steps=1, max_iterations=1, gtol=1.0)
    assert decide(lib, s, o, 0.5, solved=False) == INVALID and s.term == FAILURE
    s.gnorm = 0.5
    end(s, o, 1)
    assert (s.term, s.done, s.m_grad) == (FAILURE, 1, INF)


def test_margin_helper(lib):
    for a, thr in ((0.5, 1.0), (3.0, 1.0), (1.0, 1.0), (0.0, 0.0), (0.0, 1e-10), (1e-300, 0.0), (-2.0, 1.0), (7.0, -3.0)):
        assert lib.dsm_tr_margin(a, thr) == margin(a, thr)
    assert lib.dsm_tr_margin(0.0, 0.0) == 0.0
    for a in (INF, -INF, NAN):
        assert lib.dsm_tr_margin(a, 1.0) == INF  # not a decision that rounding can flip
    assert math.isnan(lib.dsm_tr_margin(1.0, NAN))


def test_every_margin_keeps_its_minimum_and_never_takes_a_nan(lib):
    ptol, ftol, x2 = 2.0 ** -10, 2.0 ** -4, 9.0
    s, o = start(lib, cost=8.0, ptol=ptol, ftol=ftol, gtol=1.0)
    thr = ptol * (math.sqrt(x2) + ptol)
    want = dict(m_accept=INF, m_grad=INF, m_func=INF, m_param=INF)
    cost = 8.0
    # a far step, a close one, a far one again: every margin falls and then stays
    for cand, mcc, step2, gnorm in ((1.0, 2.0, 4.0, 9.0), (0.9, 1.0, 1e-4, 1.25), (0.5, 1.0, 25.0, 100.0)):
        code = decide(lib, s, o, cand, mcc=mcc, step2=step2, x2=x2)
        want["m_param"] = min(want["m_param"], margin(math.sqrt(step2), thr))
        want["m_func"] = min(want["m_func"], margin(abs(cost - cand), ftol * cost))
        want["m_accept"] = min(want["m_accept"], abs((cost - cand) - 1e-3 * mcc) / max(cost, DBL_MIN))
        assert code == ACCEPTED
        cost = cand
        s.gnorm = gnorm
        lib.dsm_tr_end_iteration(s, o, 1)
        want["m_grad"] = min(want["m_grad"], margin(gnorm, 1.0))
        assert {k: getattr(s, k) for k in want} == want and s.done == 0
    # the same calls with every threshold NaN: each candidate margin is NaN and replaces nothing
    before = dict(want)
    o.ptol = o.ftol = o.min_relative_decrease = o.gtol = NAN
    assert decide(lib, s, o, 0.25, step2=1.0, x2=x2) == REJECTED  # rho > NaN is false
    s.gnorm = 0.5
    lib.dsm_tr_end_iteration(s, o, 1)
    assert {k: getattr(s, k) for k in want} == before and s.done == 0
    # and on a state that has recorded nothing yet
    s, o = start(lib, ptol=NAN, ftol=NAN, min_relative_decrease=NAN, gtol=NAN)
    assert decide(lib, s, o, 0.5) == REJECTED
    s.gnorm = 0.5
    lib.dsm_tr_end_iteration(s, o, 1)
    assert (s.m_accept, s.m_grad, s.m_func, s.m_param) == (INF,) * 4
