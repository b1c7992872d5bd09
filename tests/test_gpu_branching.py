"""BranchingProcesses on the GPU, every route at the shapes where its kernels can go wrong: the four routes of run_branching
(one launch / a launch per date / binned / XCD-affine) forced through mcg_debug_branch_route with 256-path slices, so that a
ragged last tile, a lone live lane in a workgroup, exactly sixteen bins, the raised slice shift and every quad boundary of the
branch count are reached at a few thousand paths.  Every price is compared with the oracle in philox mode (the same resampling
draws) at the pricer's bar, rtol 1e-12 / atol 1e-14 on (price, lower, upper); the routes differ only in the order in which a
path's branch values are added."""
import numpy as np
import pytest

import montecarlooptionspricer_amd as mc

pytestmark = pytest.mark.gpu

SEED, PRICE_SEED = 20260117, 41
STEPS, DT, PATH_BEGIN = 6, 1.0 / 252.0, 6
SHIFT = 8                                  # 256-path slices
ONE_LAUNCH, PER_DATE, BINNED, XCD = 1, 2, 3, 4
LISTS = {"all": np.arange(STEPS), "sparse": [0, 2, 3, 5],
         "shuffled": [4, 1, 5, 0, 2],      # its last entry, not its largest, ends the branching
         "lastcol": [0, 2, 4, STEPS]}      # ends on the last column: t_idx + 1 == n_cols, no continuation there
# per route: the sizes that are its edges (the first ragged one serves the branch-count and list cases)
SIZES = {ONE_LAUNCH: [1025, 1, 255, 257, 2049],      # 1025: a second workgroup with one live lane; 2049: eight slices and one path -> shift 9
         PER_DATE: [600, 1, 1024, 1025, 2049],       # 3 slices ragged; 4 slices exactly; 5; 9 -> the shift is raised to 9
         BINNED: [3001, 769, 4096, 4097],            # 12 slices; 256 * 3 + 1; 16 slices exactly (the high six-bit fields); 17 -> raised
         XCD: [513, 1, 1024, 3001]}                  # one tile plus one path; a lone path; two tiles exactly; six tiles, ragged
BRANCHES = [1, 3, 4, 5, 8, 9, 12]                     # the quad boundaries, all three QUADS instantiations


@pytest.fixture(scope="module")
def eng():
    e = mc.PathEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def orc():
    from oracle.binding import Oracle
    return Oracle()


@pytest.fixture(scope="module")
def paths(eng):
    """n -> (device matrix, its host copy), generated once per size"""
    made = {}

    def get(n):
        if n not in made:
            P = eng.gbm(SEED, 100.0, 0.04, 0.3, DT, STEPS, n, path_begin=PATH_BEGIN)
            made[n] = (P, P.to_host_step_major())
        return made[n]

    yield get
    for P, _ in made.values():
        P.free()


def check(eng, orc, paths, route, n, branches, ex_kind, want_route=None):
    P, host = paths(n)
    ex = np.asarray(LISTS[ex_kind], dtype=np.int32)
    eng.debug_branch_route(route, SHIFT)
    try:
        # a put that matures on the last date; a call whose maturity cuts the list (the reference's `t > maturity` break)
        for is_call, maturity in ((False, STEPS * DT), (True, (STEPS - 1.5) * DT)):
            got = eng.price_branching(P, 0.04, 100.0, maturity, DT, is_call, branches, ex, seed=PRICE_SEED)
            assert eng.debug_branch_route() == (route if want_route is None else want_route)
            want = orc.branching_price(host, 0.04, 100.0, maturity, DT, is_call, branches, ex, PRICE_SEED, mode="philox",
                                       path_begin=PATH_BEGIN)
            assert np.allclose(got, want, rtol=1e-12, atol=1e-14), (route, n, branches, ex_kind, is_call, got, want)
    finally:
        eng.debug_branch_route(0, 0)


@pytest.mark.parametrize("route,n", [(r, n) for r in SIZES for n in SIZES[r]])
def test_route_at_its_edge_sizes(eng, orc, paths, route, n):
    check(eng, orc, paths, route, n, 10, "all")


@pytest.mark.parametrize("branches", BRANCHES)
@pytest.mark.parametrize("route", list(SIZES))
def test_route_at_every_quad_boundary(eng, orc, paths, route, branches):
    check(eng, orc, paths, route, SIZES[route][0], branches, "sparse")


@pytest.mark.parametrize("ex_kind", list(LISTS))
@pytest.mark.parametrize("route", list(SIZES))
def test_route_on_every_exercise_list(eng, orc, paths, route, ex_kind):
    check(eng, orc, paths, route, SIZES[route][0], 7, ex_kind)


@pytest.mark.parametrize("route", list(SIZES))
def test_thirteen_branches_fall_back_to_one_launch(eng, orc, paths, route):
    """more than twelve branches: no route keeps the indices, the plan takes k_branch_bounds_any whatever is asked for"""
    check(eng, orc, paths, route, SIZES[route][0], 13, "all", want_route=ONE_LAUNCH)


def test_default_shift_and_automatic_route(eng, orc, paths):
    """route 0 with the default slices: a few thousand paths are one slice, one launch; with 256-path slices the plan itself
    chooses the per-date route (3 slices) and the binned one (12 slices)"""
    for n, shift, want_route in ((3001, 0, ONE_LAUNCH), (600, SHIFT, PER_DATE), (3001, SHIFT, BINNED)):
        P, host = paths(n)
        eng.debug_branch_route(0, shift)
        try:
            got = eng.price_branching(P, 0.04, 100.0, STEPS * DT, DT, False, 10, LISTS["all"], seed=PRICE_SEED)
            assert eng.debug_branch_route() == want_route
        finally:
            eng.debug_branch_route(0, 0)
        want = orc.branching_price(host, 0.04, 100.0, STEPS * DT, DT, False, 10, LISTS["all"], PRICE_SEED, mode="philox",
                                   path_begin=PATH_BEGIN)
        assert np.allclose(got, want, rtol=1e-12, atol=1e-14), (n, shift, got, want)


def test_hook_arguments(eng):
    last = eng.debug_branch_route()                      # a query changes nothing
    assert eng.debug_branch_route(-1, 99) == last        # (nor does it look at the shift)
    for bad in ((5, 0), (-2, 0), (1, -1), (1, 31)):
        with pytest.raises(mc.McgError):
            eng.debug_branch_route(*bad)
    assert eng.debug_branch_route() == last


@pytest.mark.parametrize("route", list(SIZES))
def test_no_paths_with_a_route_forced(route):
    """An empty shard never reaches a per-date kernel (they clamp dead lanes to path n - 1): the plan chooses, the one-launch
    kernel takes its early-out, and the call fails with the reference's message.  With a collective installed (here: a world
    of one rank, whose sum is the identity) the empty shard goes all the way to the sums; without one the entry point
    refuses it at once."""
    e = mc.PathEngine(0)
    try:
        e.set_allreduce(lambda buf, count, stream: None)
        P = e.gbm(SEED, 100.0, 0.04, 0.3, DT, STEPS, 0, path_begin=PATH_BEGIN)
        e.debug_branch_route(route, SHIFT)
        with pytest.raises(mc.McgError, match="BranchingProcesses: Empty pricePaths."):
            e.price_branching(P, 0.04, 100.0, STEPS * DT, DT, False, 10, LISTS["all"], seed=PRICE_SEED)
        assert e.debug_branch_route() == ONE_LAUNCH
        e.set_allreduce(None)
        with pytest.raises(mc.McgError, match="BranchingProcesses: Empty pricePaths."):
            e.price_branching(P, 0.04, 100.0, STEPS * DT, DT, False, 10, LISTS["all"], seed=PRICE_SEED)
        P.free()
    finally:
        e.close()
