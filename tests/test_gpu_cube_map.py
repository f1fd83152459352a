"""The pooled cube map of csrc/mapping.hip (k_map_rank, k_map_gather, k_map_new, k_new_scatter, k_cube_bounds, k_cube_vox_keys, k_heads64,
k_cube_centroids and the host bookkeeping around them: MakeValidSet, LayoutMatches, StepWindow, UpdateLaunch / UpdateFinish, GetCube /
GetCloud) against the CPU oracle AND the plain model of tests/cube_map_ref.py, to the bit, point order included.

At a pose the caller states the cube map is integer bookkeeping plus fp32 arithmetic in a fixed order (the library is built with
-ffp-contract=off), so every comparison here is of bytes: the centre, the valid list in the order lio_map_get_cube_state returns it (the
selection loop's: i outermost, k innermost), the from-map clouds, and the cubes.  The cases, what each is for and the runner are in
tests/cube_map_cases.py; tests/test_cube_map_ref.py holds the model to the oracle without a GPU."""
import numpy as np
import pytest

import cube_map_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def references(oracle):
    cache = {}

    def get(name):
        if name not in cache:
            orc = cases.play_case(cases.CASES[name](), cases.lib_handles(oracle), "oracle")
            model = None if name in cases.NO_MODEL else cases.play_case(cases.CASES[name](), cases.model_handles, "model")
            cache[name] = (orc, model)
        return cache[name]

    return get


@pytest.mark.parametrize("name", list(cases.CASES))
def test_cube_map_bits(hip, references, name):
    """Every snapshot of the case: "all" ones read all 4851 indices of both classes from the product, the others every cube the oracle
    has points in and all neighbours of those (a point filed one cube off shows twice).  The ops only the product has (126 valid cubes,
    a pose beyond the packed cube keys) must return LIO_ERR_CAPACITY and leave every cube, cloud and list as it was: the runner compares
    all of them before and after, so a getter that answered with aliased cubes would show."""
    orc, model = references(name)
    got = cases.play_case(cases.CASES[name](), cases.lib_handles(hip), "product", probes=cases.near_probes(orc))
    cases.same_run(orc, got, f"{name}: oracle vs product")
    if model is not None:
        cases.same_run(model, got, f"{name}: model vs product")


def test_one_handle_through_shift_and_relayout(hip, oracle):
    """`shift` and then `relayout` on the SAME handle: the relayout's lists arrive at a moved centre, over a pool the walk has emptied and
    refilled, with whatever layout state the walk left."""
    ops = cases.shift_ops() + cases.relayout_ops()
    orc = cases.play(ops, cases.LibMap(oracle, {}), "oracle")
    model = cases.play(ops, cases.model_handles({}), "model")
    got = cases.play(ops, cases.LibMap(hip, {}), "product", probes=cases.near_probes(orc))
    cases.same_run(orc, got, "shift + relayout: oracle vs product")
    cases.same_run(model, got, "shift + relayout: model vs product")


def test_process_batch_of_two_equals_one_by_one(hip, oracle):
    """Two handles through lio_map_process_batch against two handles stepped one by one (and the oracle): small maps, so every step is the
    association, the stacks' round trip and filters, the window, the selection and the map update, and the poses are the same bits."""
    from lio_amd import capi

    rng = np.random.default_rng(30)
    small = ((-20.0, -20.0, -5.0), (20.0, 20.0, 5.0))
    steps = []
    for t0, t1 in (((0.0, 0.0, 0.0), (0.25, 0.5, 0.0)), ((0.5, -0.25, 0.125), (600.0, 0.0, -64.0)), ((1.5, 2.0, -0.75), (0.0, 64.0, 0.0))):
        steps.append([(cases.box(rng, 3, *small, first_intensity=100.0), cases.box(rng, 150, *small, first_intensity=200.0), (cases.IDENT, t0)),
                      (cases.box(rng, 2, *small, first_intensity=300.0), cases.box(rng, 257, *small, first_intensity=400.0), (cases.IDENT, t1))])
    poses = [[(cases.HALF_X, (17.7, -8.8, 0.4)), (cases.IDENT, (610.4, 23.1, 3.6))], [(cases.IDENT, (10.4, 23.1, 3.6)), (cases.GENERIC_Q, (643.7, 73.8, 16.1))]]
    batch = [cases.LibMap(hip, {}), cases.LibMap(hip, {})]
    single = [cases.LibMap(hip, {}), cases.LibMap(hip, {})]
    orc = [cases.LibMap(oracle, {}), cases.LibMap(oracle, {})]

    def compare(what, with_stacks, kind="near"):
        for k in range(2):
            o = cases.read(orc[k], "all", with_stacks=with_stacks)
            probe = cases.near_probes([o])[0]
            a = cases.read(single[k], kind, probe, with_stacks=with_stacks)
            cases.same(a, cases.read(batch[k], kind, probe, with_stacks=with_stacks), f"{what}, handle {k}: one by one vs batch")
            cases.same(o, a, f"{what}, handle {k}: oracle vs product")

    for n, inputs in enumerate(steps):
        for k in range(2):
            batch[k]._grow(*inputs[k][:2])
            for side in (single, orc):
                side[k].set_init_flag(False)
                assert side[k].process(*inputs[k]) == cases.LIO_OK
        capi.PointMapping.process_batch([h.m for h in batch], inputs)
        compare(f"step {n}", True)
    empty = (cases.EMPTY, cases.EMPTY, cases.ID)
    for n, qp in enumerate(poses):
        for k in range(2):
            for side in (single, orc, batch):
                side[k].set_init_flag(True)
                side[k].set_transform_tobe_mapped(*qp[k])
            for side in (single, orc):
                assert side[k].process(*empty) == cases.LIO_OK
        capi.PointMapping.process_batch([h.m for h in batch], [empty, empty])
        compare(f"pose {n}", False, "all" if n == len(poses) - 1 else "near")
    assert len(batch[1].cloud(3)) > 0 and len(batch[0].cloud(3)) > 0
