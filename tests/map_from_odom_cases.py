"""The rig of the tests of include/lio_map_from_odom.h (tests/test_gpu_map_from_odom.py).

The raw sweeps are those of tests/frontend_batch_cases.py.  Every sweep goes through the product's PointProcessor and
lio_odom_process_batch_from_pp ONCE per step; the odometry handles (`sources`) then feed twin sets of map handles: `fed` by the route under
test (lio_map_process_batch_from_odom), `host` by the host route the header states as the contract — lio_odom_get_last_cloud twice, the
transform_sum the odometry's last call wrote, lio_pp_get_cloud(RINGS) -> lio_odom_full_to_end -> lio_map_set_full_cloud, then
lio_map_process_batch.  Every comparison is on uint32 views, no tolerance, over the state tests/test_gpu_map_batch.py compares (the full
cloud is part of it).

A map handle is a dict: name, src (the source that feeds it), cfg (overrides of lio_map_default_config), init_at (the step before which
lio_map_set_init_flag(h, 1) is called, or None), pp (the source whose processor supplies its full cloud; None: no full cloud).
"""
import numpy as np

from lio_amd import capi
import frontend_batch_cases as fbc

RINGS = 0


def bits(a):
    if isinstance(a, tuple):                                     # a transform: (q_xyzw, p)
        a = np.concatenate([np.asarray(x, np.float32).ravel() for x in a])
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def map_handle(name, src, pp="same", init_at=None, **cfg):
    return dict(name=name, src=src, pp=src if pp == "same" else pp, init_at=init_at, cfg=cfg)


def one_each(fronts, **cfg):
    """one default map handle per source, full cloud on"""
    return [map_handle(f["name"], j, **cfg) for j, f in enumerate(fronts)]


def map_state(m):
    """everything a map handle answers after a step (tests/test_gpu_map_batch.py::_state)"""
    cen, valid = m.cube_state()
    score, point, coeff = m.score_point_coeff()
    st = dict(tobe=bits(m.transform_tobe_mapped()), cen=np.array(cen, np.int32), valid=valid, score=score, point=point, coeff=coeff,
              surround=m.surround(0.6), full=m.full_cloud())
    for w in range(4):
        st[f"cloud{w}"] = m.cloud(w)
    for idx in valid:
        for c in range(2):
            st[f"cube{c}_{int(idx)}"] = m.cube(c, idx)
    return st


def assert_same(a, b, what):
    assert a.keys() == b.keys(), (what, sorted(set(a) ^ set(b)))
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape, (what, k, x.shape, y.shape)
        if x.dtype.kind == "f":
            x, y = bits(x), bits(y)
        assert np.array_equal(x, y), (what, k)


def assert_same_result(ra, rb, what):
    assert np.array_equal(bits(ra["T_aft"]), bits(rb["T_aft"])), (what, "T_aft")
    for k in ("iterations", "num_selected", "degenerate", "kz"):
        assert ra[k] == rb[k], (what, k, ra[k], rb[k])


def full_257():
    return np.ascontiguousarray(fbc.raw("indoor", fbc.T0S[0], 2)[0][1][:257])


def odom_snapshot(od, full):
    """what every accessor of an odometry handle answers"""
    trace, kz = od.iteration_trace()
    return [bits(od.last_cloud(0)), bits(od.last_cloud(1)), bits(trace), np.array([kz]), bits(od.full_to_end(full))]


def pp_snapshot(pp):
    """what the accessors of a processor answer (tests/test_gpu_frontend_batch.py::_snapshot, and the ring-ordered cloud)"""
    out = [bits(pp.cloud(w)) for w in (0, 1, 2, 3, 4)]
    for w in (1, 2, 3):
        out += list(pp.indices(w))
    return out


def assert_snapshots_equal(a, b, what):
    assert len(a) == len(b), what
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and np.array_equal(x, y), (what, i)


def each_alone(pps, sweeps):
    for pp, x in zip(pps, sweeps):
        pp.process(x)


def pooled(pps, sweeps):
    """the sweeps of every group of equal ring counts through one lio_pp_process_batch (a group of one keeps its own storage)"""
    groups = {}
    for p, pp in enumerate(pps):
        groups.setdefault(pp.rings, []).append(p)
    for members in groups.values():
        if len(members) > 1:
            capi.PointProcessor.process_batch([pps[p] for p in members], [sweeps[p] for p in members])
        else:
            pps[members[0]].process(sweeps[members[0]])


class Rig:
    """sources (a processor and an odometry handle per sensor of frontend_batch_cases) and the twin sets of map handles they feed"""

    def __init__(self, hip, fronts, maps=None, twin_odoms=False):
        self.hip, self.fronts = hip, fronts
        self.maps = one_each(fronts) if maps is None else maps
        self.full = full_257()
        self.pps = [capi.PointProcessor(hip, f["lidar"].lower_deg, f["lidar"].upper_deg, f["lidar"].rings) for f in fronts]
        self.ods = [capi.PointOdometry(hip, *f["params"]) for f in fronts]
        self.ods_twin = [capi.PointOdometry(hip, *f["params"]) for f in fronts] if twin_odoms else None   # never handed to the call under test
        self.last = [None] * len(fronts)                        # what the odometry's last process call returned
        for j, f in enumerate(fronts):
            for x in f["prep"]:
                self.pps[j].process(x)
                cl = [self.pps[j].cloud(w) for w in (1, 2, 3, 4)]
                self.last[j] = self.ods[j].process(*cl)
                if twin_odoms:
                    self.ods_twin[j].process(*cl)
            if f["disable"]:
                self.ods[j].enable(False)
                if twin_odoms:
                    self.ods_twin[j].enable(False)
        self.fed = [capi.PointMapping(hip, **m["cfg"]) for m in self.maps]
        self.host = [capi.PointMapping(hip, **m["cfg"]) for m in self.maps]
        self.counts = []                                         # per step and map handle: (n_corner, n_surf, n_full or None)

    # ---- the front end: one sweep per source
    def feed(self, k, feed=each_alone):
        feed(self.pps, [f["steps"][k] for f in self.fronts])
        self.last = capi.PointOdometry.process_batch_from_pp(self.ods, self.pps)
        if self.ods_twin is not None:                            # the twins took no part in any lio_map_process_batch_from_odom
            rt = capi.PointOdometry.process_batch_from_pp(self.ods_twin, self.pps)
            for j, f in enumerate(self.fronts):
                fbc.same(fbc.state(self.ods[j], self.last[j], self.full), fbc.state(self.ods_twin[j], rt[j], self.full), (f["name"], "odometry twin", k))

    def snapshot_sources(self):
        return [odom_snapshot(od, self.full) for od in self.ods], [pp_snapshot(pp) for pp in self.pps]

    # ---- the host route of the contract for map handle j
    def host_input(self, j):
        od = self.ods[self.maps[j]["src"]]
        return od.last_cloud(0), od.last_cloud(1), self.last[self.maps[j]["src"]]["T_sum"]

    def unregistered_full(self, j):
        m = self.maps[j]
        return self.ods[m["src"]].full_to_end(self.pps[m["pp"]].cloud(RINGS))

    def host_route(self, handles, order, with_pp, alone=False):
        inputs = []
        for j in order:
            if with_pp[j]:
                handles[j].set_full_cloud(self.unregistered_full(j))   # (an empty cloud clears it)
            inputs.append(self.host_input(j))
        if alone:
            return [handles[j].process(*inp) for j, inp in zip(order, inputs)]
        return capi.PointMapping.process_batch([handles[j] for j in order], inputs)

    def new_route(self, handles, order, with_pp, no_pp_array=False):
        pps = None if no_pp_array else [self.pps[self.maps[j]["pp"]] if with_pp[j] else None for j in order]
        return capi.PointMapping.process_batch_from_odom([handles[j] for j in order], [self.ods[self.maps[j]["src"]] for j in order], pps)

    # ---- one step of every map handle
    def step(self, k, feed=each_alone, how="new", order=None, with_pp=None, no_pp_array=False):
        """sweep k through the front end, then every map handle one step: `fed` as `how` says ('new': the call under test, 'batch' /
        'alone': the host route through lio_map_process_batch / lio_map_process), `host` by the host route -> the host results per handle.
        with_pp[j] False: handle j takes no full cloud this step; no_pp_array: pp_or_null is NULL."""
        n = len(self.maps)
        self.feed(k, feed)
        order = list(range(n)) if order is None else order
        with_pp = [m["pp"] is not None for m in self.maps] if with_pp is None else with_pp
        if no_pp_array:
            with_pp = [False] * n
        for j, m in enumerate(self.maps):
            if m["init_at"] == k:
                self.fed[j].set_init_flag(True), self.host[j].set_init_flag(True)
        before = self.snapshot_sources()
        if how == "new":
            rf = self.new_route(self.fed, order, with_pp, no_pp_array)
        else:
            rf = self.host_route(self.fed, order, with_pp, alone=(how == "alone"))
        after = self.snapshot_sources()
        for name, b, a in zip(("odometry", "processor"), before, after):   # the sources are only read
            for j, (x, y) in enumerate(zip(b, a)):
                assert_snapshots_equal(x, y, (name, "changed", j, "step", k))
        rh = self.host_route(self.host, list(range(n)), with_pp)
        out = [None] * n
        for pos, j in enumerate(order):
            out[j] = rf[pos]
        cnt = []
        for j, m in enumerate(self.maps):
            what = (m["name"], j, "step", k, how)
            assert_same_result(rh[j], out[j], what)
            assert_same(map_state(self.host[j]), map_state(self.fed[j]), what)
            c, s, _ = self.host_input(j)
            cnt.append((len(c), len(s), len(self.pps[m["pp"]].cloud(RINGS)) if with_pp[j] else None))
        self.counts.append(cnt)
        return rh
