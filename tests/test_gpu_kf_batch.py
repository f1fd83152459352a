"""GPU parity of the batched keyframe refinement (BASELINE.json configs[4]) through the C-ABI: every keyframe of a
batch advanced by the three per-round launches must land where the oracle's sequential scan-to-map loop lands."""
import numpy as np
import pytest

from lio_amd import capi
from kf_util import keyframe_inputs, load

pytestmark = pytest.mark.gpu

POS_TOL = 1e-4   # m   (north-star tolerance)
ROT_TOL = 1e-4   # rad (quaternion components: half-angle, stricter)


def _assert_batches_agree(rh, ro, noisy_fraction=0.0):
    """Poses within the north-star tolerance after the same iteration count.  The loop exits when a step falls below
    0.05 cm / 0.05 deg (PointMapping.cc:714-716): a keyframe whose deciding step sits on that threshold may take one
    round more or less when the fp32 sums are ordered differently; those are counted (few allowed) and bounded by the
    size of the step they skipped."""
    same = rh["iterations"] == ro["iterations"]
    assert np.all(np.abs(rh["iterations"] - ro["iterations"]) <= 1)
    assert np.count_nonzero(~same) <= max(1, len(same) // 10), (rh["iterations"], ro["iterations"])
    assert np.max(np.abs(rh["rows"] - ro["rows"])[same]) <= max(3, int(ro["rows"].max()) // 500)
    dp = np.abs(rh["p"] - ro["p"]).max(axis=1)
    dq = np.minimum(np.abs(rh["q"] - ro["q"]).max(axis=1), np.abs(rh["q"] + ro["q"]).max(axis=1))
    tight = same & (dp < POS_TOL) & (dq < ROT_TOL)
    # noisy_fraction > 0 (4-DoF only): MapBuilder::OptimizeMap scales the roll / pitch columns by 5e-3 (MapBuilder.cc:903-914), which
    # leaves some 6x6 systems numerically singular in fp32; Eigen's colPivHouseholderQr().solve keeps a pivot unless it is essentially
    # exactly zero ((max norm * eps)^2 (rows - k) / rows, tests/golden/README.md), so the weak unknown of such a system is rounding
    # noise over a tiny pivot in ANY implementation.  Those keyframes are counted and bounded instead (measured: 2 of 12 at 1.8e-4 m).
    print(f"keyframe batch vs oracle: {int(np.count_nonzero(same))} of {len(same)} keyframes with equal iteration counts, worst |dp| {dp[same].max():.2e} m, |dq| {dq[same].max():.2e}; "
          f"{int(np.count_nonzero(same & ~tight))} beyond 1e-4 (allowed {int(noisy_fraction * len(same))}); others: " +
          (f"|dp| {dp[~same].max():.2e} |dq| {dq[~same].max():.2e}" if np.any(~same) else "none"))
    assert np.count_nonzero(same & ~tight) <= int(noisy_fraction * len(same)), (dp, dq)
    # caps at ~2x what the MI355X measures (round 6): 6-DoF 8.6e-6 m / 1.2e-7; 4-DoF 1.76e-4 m / 1.8e-6 on the two keyframes whose
    # 6 x 6 system is numerically singular in fp32 (see above) — that class cannot be held to 1e-4 by any fp32 implementation
    cap_p, cap_q = (3e-4, 1e-5) if noisy_fraction > 0 else (2e-5, 1e-6)
    assert dp[same].max() < cap_p and dq[same].max() < cap_q, (dp[same].max(), dq[same].max())
    if np.any(~same):
        assert dp[~same].max() < 1e-3 and dq[~same].max() < 1e-3


@pytest.mark.parametrize("four_dof", [0, 1])
def test_batch_matches_oracle_vlp16(hip, oracle, four_dof):
    maps, kfs = keyframe_inputs(oracle, "indoor", 4, 4)
    bh = load(capi.KeyframeBatch(hip, map_builder=four_dof, enable_4d=four_dof), maps, kfs)
    bo = load(capi.KeyframeBatch(oracle, map_builder=four_dof, enable_4d=four_dof), maps, kfs)
    rh, ro = bh.refine(), bo.refine()
    assert rh["device_ms"] > 0
    _assert_batches_agree(rh, ro, noisy_fraction=0.25 if four_dof else 0.0)
    # repeatable, and independent of the batch a keyframe sits in
    rh2 = bh.refine()
    np.testing.assert_array_equal(rh["p"], rh2["p"])
    np.testing.assert_array_equal(rh["q"], rh2["q"])
    one = capi.KeyframeBatch(hip, map_builder=four_dof, enable_4d=four_dof)
    one.add_map(*maps[kfs[7][0]])
    one.add_keyframe(0, kfs[7][1], kfs[7][2], kfs[7][3])
    r1 = one.refine()
    np.testing.assert_array_equal(r1["p"][0], rh["p"][7])
    np.testing.assert_array_equal(r1["q"][0], rh["q"][7])


def _assert_twin(hip, mh, r, T0, **batch_kw):
    """the handle's last process against a batch of one keyframe built from the handle's own clouds and start pose: the same bits"""
    b = capi.KeyframeBatch(hip, **batch_kw)
    b.add_map(mh.cloud(capi.PointMapping.CORNER_FROM_MAP), mh.cloud(capi.PointMapping.SURF_FROM_MAP))
    b.add_keyframe(0, mh.cloud(capi.PointMapping.CORNER_STACK_DS), mh.cloud(capi.PointMapping.SURF_STACK_DS), T0)
    rb = b.refine()
    assert rb["iterations"][0] == r["iterations"] and rb["rows"][0] == r["num_selected"]
    np.testing.assert_array_equal(rb["p"][0], r["T_aft"][1])
    np.testing.assert_array_equal(rb["q"][0], r["T_aft"][0])


def test_batch_equals_single_keyframe_handle(hip, oracle):
    """The scan-to-map handle runs the batch's launch chain on a table of one keyframe (csrc/mapping.hip: MapChain::Iterate on a chain
    of one), so the two agree by construction; what this still guards is everything around the chain — the handle's table (grids,
    stack, start state in one upload), the per-sensor mailboxes it reads behind rounds 6, 8 and 10 where the batch reads its
    convergence count, and the batch's query order and lane split.  Refine shares no host code with the handle.  Three cuts of
    the stacks: full; no corner point (the corner half of the round launch has no block to run); 3 corner + 20 surf points (fewer
    than 50 rows every round: the loop runs dry through all three peeks and the start pose comes back untouched)."""
    from mapping_util import drifting_inputs
    frames = drifting_inputs(oracle, "indoor", 3)
    mh = capi.PointMapping(hip)
    for corner, surf, T_sum, _ in frames[:2]:
        mh.process(corner, surf, T_sum)
    mh.set_init_flag(True)                     # keeps transform_tobe_mapped as the start pose, no map update
    corner, surf, T_sum, _ = frames[2]
    max_it = mh.cfg.num_max_iterations
    for name, c, s_ in [("full", corner, surf), ("no corner", corner[:0], surf), ("dry", corner[:3], surf[:20])]:
        T0 = mh.transform_tobe_mapped()
        r = mh.process(c, s_, T_sum)
        print(f"twin {name}: stack {len(mh.cloud(0))} + {len(mh.cloud(1))}, iterations {r['iterations']}, rows {r['num_selected']}")
        if name == "no corner":
            assert len(mh.cloud(capi.PointMapping.CORNER_STACK_DS)) == 0 and r["num_selected"] >= 50
        if name == "dry":
            # iterations is the count the mailbox carried at the LAST peek (round 10); a loop that never converges passes the peeks at 6 and 8 first
            assert r["iterations"] == max_it == 10 and r["num_selected"] < 50
            np.testing.assert_array_equal(r["T_aft"][0], T0[0])
            np.testing.assert_array_equal(r["T_aft"][1], T0[1])
        _assert_twin(hip, mh, r, T0)


def test_batch_equals_map_builder_handle_4dof(hip, oracle):
    """The 4-DoF route (MapBuilder::OptimizeMap) against KeyframeBatch(map_builder=1, enable_4d=1).  A MapBuilder handle associates
    transform_sum with the map at every process, so its start pose is read from a probe: a second handle with an EMPTY map brought to
    the same (transform_bef_mapped, transform_tobe_mapped), which runs the same association on the same transform_sum and then returns
    before the optimisation (<= 10 map points: no rounds, no TransformUpdate), leaving the start pose in transform_tobe_mapped."""
    from mapping_util import drifting_inputs
    kw = dict(map_builder=1, enable_4d=1, skip_count=1)
    frames = drifting_inputs(oracle, "indoor", 3)
    none = np.zeros((0, 4), np.float32)
    mh, probe = capi.PointMapping(hip, **kw), capi.PointMapping(hip, **kw)
    for corner, surf, T_sum, _ in frames[:2]:
        r1 = mh.process(corner, surf, T_sum)
    assert r1["iterations"] > 0                 # the second sweep was optimised: transform_bef_mapped = its transform_sum (TransformUpdate)
    probe.process(none, none, frames[1][2])     # first call: transform_bef_mapped = transform_sum of sweep 1
    probe.set_transform_tobe_mapped(*mh.transform_tobe_mapped())
    corner, surf, T_sum, _ = frames[2]
    rp = probe.process(none, none, T_sum)
    assert rp["iterations"] == 0
    T0 = probe.transform_tobe_mapped()
    r = mh.process(corner, surf, T_sum)
    print(f"twin 4-DoF: iterations {r['iterations']}, rows {r['num_selected']}")
    assert r["iterations"] > 0 and r["num_selected"] >= 50
    _assert_twin(hip, mh, r, T0, map_builder=1, enable_4d=1)


def test_batch_edge_cases(hip, oracle):
    maps, kfs = keyframe_inputs(oracle, "indoor", 2, 1)
    res = []
    for lib in (hip, oracle):
        b = capi.KeyframeBatch(lib)
        tiny = b.add_map(maps[0][0][:10], maps[0][1][:100])
        ok = b.add_map(*maps[0])
        _, cs, ss, T0, _ = kfs[0]
        b.add_keyframe(tiny, cs, ss, T0)
        b.add_keyframe(ok, np.zeros((0, 4), np.float32), np.zeros((0, 4), np.float32), T0)
        b.add_keyframe(ok, cs, ss, T0)
        b.add_keyframe(ok, cs[:3], ss[:20], T0)     # < 50 rows per round: pose untouched, loop runs dry
        with pytest.raises(capi.LioError):
            b.add_keyframe(9, cs, ss, T0)
        res.append(b.refine())
        b.clear_keyframes()
        assert len(b) == 0 and b.refine()["p"].shape == (0, 3)
    rh, ro = res
    _assert_batches_agree(rh, ro)
    assert list(rh["iterations"][[0, 1, 3]]) == [0, 10, 10]
    for k in (0, 1, 3):
        np.testing.assert_array_equal(rh["p"][k], kfs[0][3][1])


def test_batch_hdl64_many_keyframes(hip, oracle):
    """64-line keyframes, 48 in one batch over 2 local maps; the oracle checks a sample of them."""
    maps, kfs = keyframe_inputs(oracle, "outdoor", 3, 24, dpos=0.15, drot=0.01)
    bh = load(capi.KeyframeBatch(hip), maps, kfs)
    rh = bh.refine()
    sample = [0, 5, 23, 24, 30, 47]
    bo = capi.KeyframeBatch(oracle)
    for mi, (cm, sm) in enumerate(maps):
        bo.add_map(cm, sm)
    for k in sample:
        bo.add_keyframe(*kfs[k][:4])
    ro = bo.refine()
    sub = {key: (rh[key][sample] if key != "device_ms" else rh[key]) for key in rh}
    _assert_batches_agree(sub, ro)
    # every perturbed copy of a keyframe comes back to the same place (within the loop's early-exit band)
    for lo in (0, 24):
        p = rh["p"][lo:lo + 24]
        assert np.max(np.linalg.norm(p[:, :2] - p[:, :2].mean(axis=0), axis=1)) < 0.02


def test_batch_larger_than_one_launch(hip, oracle):
    """More keyframes than one launch carries (grid z/y limit: 32768 per launch, kf_batch.hip): 33 000 small keyframes
    against one shared local map; a sample is checked against the oracle and every copy of a keyframe must agree with
    its twin in the other launch chunk."""
    maps, kfs = keyframe_inputs(oracle, "indoor", 2, 1)
    _, cs, ss, T0, _ = kfs[0]
    rng = np.random.default_rng(2)
    variants = []
    for _ in range(8):                                  # 8 distinct sub-sampled keyframes (>= 50 rows each round)
        variants.append((cs[rng.choice(len(cs), 40, replace=False)], ss[rng.choice(len(ss), 300, replace=False)]))
    n = 33000
    bh = capi.KeyframeBatch(hip)
    bh.add_map(*maps[0])
    for k in range(n):
        c, s_ = variants[k % 8]
        bh.add_keyframe(0, c, s_, T0)
    rh = bh.refine()
    assert len(bh) == n and rh["p"].shape == (n, 3)
    bo = capi.KeyframeBatch(oracle)
    bo.add_map(*maps[0])
    for v in range(8):
        bo.add_keyframe(0, variants[v][0], variants[v][1], T0)
    ro = bo.refine()
    first = {key: (rh[key][:8] if key != "device_ms" else rh[key]) for key in rh}
    _assert_batches_agree(first, ro)
    for v in range(8):                                   # identical inputs -> identical outputs, whichever chunk they ran in
        idx = np.arange(v, n, 8)
        assert np.all(rh["iterations"][idx] == rh["iterations"][v])
        np.testing.assert_array_equal(rh["p"][idx], np.broadcast_to(rh["p"][v], (len(idx), 3)))
        np.testing.assert_array_equal(rh["q"][idx], np.broadcast_to(rh["q"][v], (len(idx), 4)))
