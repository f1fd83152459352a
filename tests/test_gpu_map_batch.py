"""One chain of B sensors against B chains of one (include/lio_map_batch.h).  lio_map_process is lio_map_process_batch of one handle, so the
twin handles here differ in what shares a launch chain, not in the route: one set steps handle by handle (each a table of one on its own
scratch), the other in ONE call (one table, the first handle's scratch).  The same sweeps, every getter of every handle after every
step, np.array_equal on uint32 views — no tolerance.  The sensors are those of tests/map_batch_cases.py (indoor VLP-16 sweeps, a few
thousand queries each); tests/test_map_batch_abi.py shows on the CPU oracle that each kind does what its name says."""
import ctypes as C

import numpy as np
import pytest

from lio_amd import capi, pipeline
import map_batch_cases as cases

pytestmark = pytest.mark.gpu


def _bits(a):
    if isinstance(a, tuple):                                     # a transform: (q_xyzw, p)
        a = np.concatenate([np.asarray(x, np.float32).ravel() for x in a])
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _state(m):
    """everything a handle answers after a step"""
    cen, valid = m.cube_state()
    score, point, coeff = m.score_point_coeff()
    st = dict(tobe=_bits(m.transform_tobe_mapped()), cen=np.array(cen, np.int32), valid=valid, score=score, point=point, coeff=coeff,
              surround=m.surround(0.6), full=m.full_cloud())
    for w in range(4):
        st[f"cloud{w}"] = m.cloud(w)
    for idx in valid:
        for c in range(2):
            st[f"cube{c}_{int(idx)}"] = m.cube(c, idx)
    return st


def _assert_same(a, b, what):
    assert a.keys() == b.keys(), (what, sorted(set(a) ^ set(b)))
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape, (what, k, x.shape, y.shape)
        if x.dtype.kind == "f":
            x, y = _bits(x), _bits(y)
        assert np.array_equal(x, y), (what, k)


def _assert_same_result(ra, rb, what):
    assert np.array_equal(_bits(ra["T_aft"]), _bits(rb["T_aft"])), (what, "T_aft")
    for k in ("iterations", "num_selected", "degenerate", "kz"):
        assert ra[k] == rb[k], (what, k, ra[k], rb[k])


def _set_full(m, sensor, k):
    if k in sensor["full"]:
        m.set_full_cloud(sensor["full"][k])


def _twins(hip, sensors):
    return [cases.make_handle(hip, s) for s in sensors], [cases.make_handle(hip, s) for s in sensors]


def _step_alone(handles, sensors, k):
    out = []
    for m, s in zip(handles, sensors):
        _set_full(m, s, k)
        out.append(m.process(*s["steps"][k]))
    return out


def _step_batch(handles, sensors, k, order=None):
    order = list(range(len(handles))) if order is None else order
    for j in order:
        _set_full(handles[j], sensors[j], k)
    res = capi.PointMapping.process_batch([handles[j] for j in order], [sensors[j]["steps"][k] for j in order])
    out = [None] * len(handles)
    for j, r in zip(order, res):
        out[j] = r
    return out


def _compare_step(alone, batch, sensors, ra, rb, k):
    for j, s in enumerate(sensors):
        what = (s["name"], j, k)
        _assert_same_result(ra[j], rb[j], what)
        _assert_same(_state(alone[j]), _state(batch[j]), what)


def _run(hip, sensors, n_steps, how=None, orders=None):
    """twin handles through n_steps: the first set as chains of one, the second as how[k] says ('batch': one chain of all, the default) ->
    the results of the chains of one per step"""
    alone, batch = _twins(hip, sensors)
    results = []
    for k in range(n_steps):
        ra = _step_alone(alone, sensors, k)
        if how is None or how[k] == "batch":
            rb = _step_batch(batch, sensors, k, None if orders is None else orders[k])
        else:
            rb = _step_alone(batch, sensors, k)
        _compare_step(alone, batch, sensors, ra, rb, k)
        results.append(ra)
    return results, alone, batch


def test_one_sensor_through_the_batch_entry(hip, oracle):
    res, _, _ = _run(hip, [cases.moving(oracle, 0, 4)], 4)
    assert all(r[0]["iterations"] > 0 for r in res)


def test_moving_sensors_with_their_own_filter_sizes(hip, oracle):
    sensors = [cases.moving(oracle, j, 3, own_filters=True) for j in range(3)]
    res, _, _ = _run(hip, sensors, 3)
    its = [[r["iterations"] for r in step] for step in res]
    assert all(i > 0 for row in its for i in row)
    assert any(len(set(row)) > 1 for row in its), its           # converged and iterating sensors side by side in one chain


def test_all_kinds_in_one_batch(hip, oracle):
    sensors = cases.all_kinds(oracle, 2)
    res, _, batch = _run(hip, sensors, 2)
    by_name = {s["name"]: [step[j] for step in res] for j, s in enumerate(sensors)}
    max_it = batch[0].cfg.num_max_iterations
    assert [r["iterations"] for r in by_name["small_map"]] == [0, 0] and by_name["first_call"][0]["iterations"] == 0
    assert all(r["iterations"] == max_it for r in by_name["empty"] + by_name["dry"])
    assert all(r["iterations"] == 0 for r in by_name["shifted"])
    full = {s["name"]: m for s, m in zip(sensors, batch)}["full_cloud"].full_cloud()
    assert full.shape == (257, 4)


def test_map_builder_handles_that_optimise_and_skip_share_a_call(hip, oracle):
    sensors = [cases.builder(oracle, 0, 3), cases.builder(oracle, 1, 3, extra_prep=1), cases.builder(oracle, 2, 3)]
    res, _, _ = _run(hip, sensors, 3)
    its = [[r["iterations"] for r in step] for step in res]
    assert any(0 in row and max(row) > 0 for row in its), its    # a skipped call beside an optimising one


def test_mixed_peeks_in_one_chain(hip, oracle):
    """Every peek (behind rounds 6, 8 and 10) sees converged and unconverged mailboxes side by side: one sensor converges before round 6,
    one between rounds 6 and 10, and a dry one (3 corner + 20 surf points: fewer than 50 rows in every round) never does."""
    sensors = [cases.moving(oracle, 0, 2), cases.still(oracle, 0, 2), cases.dry(oracle, 2)]
    res, _, batch = _run(hip, sensors, 2)
    its = [[r["iterations"] for r in step] for step in res]
    print("iterations per step (moving0, still0, dry):", its)
    mid, early, never = its[1]
    assert early < 6 and 6 <= mid < 10 and never == batch[0].cfg.num_max_iterations, its


@pytest.mark.parametrize("kind", ["one_block", "two_blocks"])
def test_score_list_after_a_chain_of_one_and_a_chain_of_many(hip, oracle, kind):
    """The score list is read from the handle's own arrays, which the chain hands back: the same list after lio_map_process and after a
    call among other sensors, on both sides of the 2048-slot step of odom_rows_blocks, and still the same after other handles have
    used the chain that handed it back."""
    target, others = cases.blocks(oracle, kind, 1), [cases.moving(oracle, 0, 2), cases.moving(oracle, 1, 2)]
    one = cases.make_handle(hip, target)
    one.process(*target["steps"][0])
    slots = len(one.cloud(0)) + len(one.cloud(1))
    assert slots <= cases.ROW_STEP - cases.MARGIN if kind == "one_block" else slots >= cases.ROW_STEP + cases.MARGIN, slots
    want = [_bits(a) for a in one.score_point_coeff()]
    assert len(want[0]) >= 50
    first, many, last = cases.make_handle(hip, others[0]), cases.make_handle(hip, target), cases.make_handle(hip, others[1])
    capi.PointMapping.process_batch([first, many, last], [others[0]["steps"][0], target["steps"][0], others[1]["steps"][0]])
    for got, ref in zip(many.score_point_coeff(), want):
        assert np.array_equal(_bits(got), ref)
    capi.PointMapping.process_batch([first, last], [others[0]["steps"][1], others[1]["steps"][1]])   # the same chain without `many`
    other = cases.make_handle(hip, others[0])
    other.process(*others[0]["steps"][0])                                                             # ... and a chain of one of another handle
    for m in (many, one):
        for got, ref in zip(m.score_point_coeff(), want):
            assert np.array_equal(_bits(got), ref)


def test_handles_without_common_launch_parameters_fall_back(hip, oracle):
    """6-DoF, 4-DoF and another round limit share no launch parameters: the call runs a chain of one per handle, each on the handle's own
    scratch.  _run holds every handle of that call to a handle stepped alone, bit for bit, after each of two consecutive steps; the second
    step reuses every handle's own chain."""
    sensors = [cases.moving(oracle, 0, 2), cases.builder(oracle, 1, 2), cases.moving(oracle, 2, 2, num_max_iterations=3)]
    res, alone, batch = _run(hip, sensors, 2)
    assert len(res) == 2
    assert all(step[2]["iterations"] <= 3 for step in res)
    assert any(step[0]["iterations"] > 3 for step in res)       # ... so the first handle did not run under the third one's limit
    assert len({(m.cfg.map_builder, m.cfg.num_max_iterations) for m in batch}) == 3
    for j, (a, b) in enumerate(zip(alone, batch)):              # (once more after the last step, handle by handle)
        _assert_same(_state(a), _state(b), ("fall-back", j))


def test_batch_alone_batch_on_the_same_handles(hip, oracle):
    sensors = [cases.moving(oracle, j, 3) for j in range(3)] + [cases.no_corner(oracle, 3)]
    _run(hip, sensors, 3, how=["batch", "alone", "batch"])


def test_forty_copies_around_a_first_call(hip, oracle):
    one = cases.moving(oracle, 0, 2)
    sensors = [one] * 20 + [cases.first_call(oracle, 2)] + [one] * 20
    _, _, batch = _run(hip, sensors, 2)
    ref = _state(batch[0])
    for j in list(range(1, 20)) + list(range(21, 41)):
        _assert_same(ref, _state(batch[j]), ("copy", j))


def test_same_handles_a_second_time_in_reverse_order(hip, oracle):
    sensors = [cases.moving(oracle, 0, 2), cases.dry(oracle, 2), cases.moving(oracle, 1, 2), cases.blocks(oracle, "one_block", 2),
               cases.blocks(oracle, "two_blocks", 2)]
    n = len(sensors)
    _run(hip, sensors, 2, orders=[list(range(n)), list(range(n))[::-1]])


def test_refusals_leave_every_handle_as_it_was(hip, oracle):
    sensors = [cases.moving(oracle, 0, 1), cases.moving(oracle, 1, 1)]
    a, b = (cases.make_handle(hip, s) for s in sensors)
    est = capi.Estimator(hip, pipeline.config_indoor(hip, 4, 2))
    borrowed = est.map()
    inputs = [s["steps"][0] for s in sensors]

    def pose_and_cubes(m):
        cen, valid = m.cube_state()
        return _bits(m.transform_tobe_mapped()).copy(), list(cen), valid.copy()

    before = [pose_and_cubes(m) for m in (a, b, borrowed)]

    def untouched():
        for m, (pose, cen, valid) in zip((a, b, borrowed), before):
            p, c, v = pose_and_cubes(m)
            assert np.array_equal(p, pose) and c == cen and np.array_equal(v, valid)

    with pytest.raises(capi.LioError, match="code -1"):          # the same handle twice: LIO_ERR_ARG
        capi.PointMapping.process_batch([a, b, a], inputs + inputs[:1])
    untouched()
    with pytest.raises(capi.LioError, match="code -2"):          # an estimator's map: LIO_ERR_STATE
        capi.PointMapping.process_batch([a, borrowed, b], [inputs[0], inputs[1], inputs[1]])
    untouched()
    # a null cloud with a count: LIO_ERR_ARG (through ctypes: the Python view never builds one)
    H = (C.c_void_p * 2)(a.h, b.h)
    cl = [np.ascontiguousarray(x, np.float32) for x in (inputs[0][0], inputs[0][1], inputs[1][1])]
    corner = (capi.c_float_p * 2)(cl[0].ctypes.data_as(capi.c_float_p), None)
    surf = (capi.c_float_p * 2)(cl[1].ctypes.data_as(capi.c_float_p), cl[2].ctypes.data_as(capi.c_float_p))
    ncorner, nsurf = (C.c_size_t * 2)(len(cl[0]), 5), (C.c_size_t * 2)(len(cl[1]), len(cl[2]))
    Ts = (capi.TransformF * 2)(*[capi.TransformF.make(*inp[2]) for inp in inputs])
    Ta = (capi.TransformF * 2)()
    it = np.full(2, 7, np.int32)
    rc = hip.dll.lio_map_process_batch(H, 2, corner, ncorner, surf, nsurf, Ts, Ta, it.ctypes.data_as(capi.c_int32_p), None)
    assert rc == -1 and list(it) == [7, 7]
    untouched()
    # ... and the handles still step like their twins
    ra = [cases.make_handle(hip, s).process(*s["steps"][0]) for s in sensors]
    rb = capi.PointMapping.process_batch([a, b], inputs)
    for j in range(2):
        _assert_same_result(ra[j], rb[j], ("after refusals", j))
