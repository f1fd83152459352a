"""The rig of the tests of include/lio_est_from_odom.h (tests/test_gpu_est_from_odom.py).

Windows are those of tests/est_push_cases.py (twins from one seed).  A `Source` is a PointProcessor and a PointOdometry handle: fed with the
frames of the windows' own sequence it is what a sensor's front end leaves behind, fed with crafted less-sharp / less-flat clouds it holds
clouds of chosen sizes in last_corner_ / last_surf_ without a crafted sweep.  The routes: `fed` (the calls under test) and the host route
the header states as the contract — lio_odom_get_last_cloud twice, lio_pp_get_cloud(RINGS) -> lio_odom_full_to_end ->
lio_map_set_full_cloud, then lio_est_batch_push_frames / lio_est_push_frame, or lio_compact_encode -> lio_est_process_compact on a
device_solve = 1 handle.  Every comparison is on uint32 / uint64 views, no tolerance.
"""
import numpy as np

from lio_amd import capi
import est_push_cases as epc
import map_from_odom_cases as mfo

RINGS = 0
EMPTY = np.zeros((0, 4), np.float32)
ERR_ARG, ERR_STATE = -1, -2


def _processor(hip):
    lid = epc.data()[0].lidar
    return capi.PointProcessor(hip, lid.lower_deg, lid.upper_deg, lid.rings)


def scan(k):
    return epc.data()[0].frames[k].scan


def stamp(k):
    return epc.data()[0].frames[k].t


class Source:
    """a sensor's front end.  prep: the frames it has seen before the test's first step (two consecutive ones make the next step of an
    enabled odometry a publishing step: to_end set, the full cloud goes through odo_to_end_body); enabled False: lio_odom_enable(h, 0)
    behind them (packer mode: the clouds are kept as they come, the full cloud is copied)"""

    def __init__(self, hip, prep=(), enabled=True):
        self.hip, self.enabled = hip, enabled
        self.pp, self.od = _processor(hip), capi.PointOdometry(hip)
        self.last = None
        for k in prep:
            self.frame(k)
        if not enabled:
            self.od.enable(False)

    def frame(self, k):
        """frame k of the windows' sequence through the processor and the odometry"""
        self.pp.process(scan(k))
        self.last = self.od.process(*[self.pp.cloud(w) for w in (1, 2, 3, 4)])

    def crafted(self, corner, surf):
        """the odometry's next sweep with `corner` / `surf` as its less-sharp / less-flat clouds (the processor's sharp and flat ones as they are)"""
        self.last = self.od.process(self.pp.cloud(1), corner, self.pp.cloud(3), surf)

    def T_sum(self):
        return capi.TransformF.make(*self.last["T_sum"])


def host_clouds(src):
    """(corner, surf) as the host route reads them"""
    return src.od.last_cloud(0), src.od.last_cloud(1)


def host_full(src, pp):
    """lio_pp_get_cloud(RINGS) -> lio_odom_full_to_end"""
    return src.od.full_to_end(pp.cloud(RINGS))


def snapshot(sources, pps):
    full = mfo.full_257()
    return [mfo.odom_snapshot(s.od, full) for s in sources], [mfo.pp_snapshot(p) for p in pps if p is not None]


def assert_sources_unchanged(before, after, what):
    for name, b, a in zip(("odometry", "processor"), before, after):
        assert len(b) == len(a), (what, name)
        for j, (x, y) in enumerate(zip(b, a)):
            mfo.assert_snapshots_equal(x, y, (what, name, "changed", j))


def map_view(est):
    """lio_map_get_full_cloud and lio_map_get_transform_tobe_mapped of lio_est_map"""
    m = est.map()
    return dict(full=epc.bits(m.full_cloud()), full_n=np.array([len(m.full_cloud())], np.uint32), tobe=mfo.bits(m.transform_tobe_mapped()))


def assert_maps(A, B, what):
    for w, (a, b) in enumerate(zip(A, B)):
        epc.assert_same(map_view(a), map_view(b), f"{what}, map of window {w}")


def same_reports(ra, rb, what):
    for w, (a, b) in enumerate(zip(ra, rb)):
        assert epc.rep_key(a) == epc.rep_key(b), (what, w, epc.rep_key(a), epc.rep_key(b))


def imu(ests, k):
    for e in ests:
        epc.imu(e, k)


# ---------------------------------------------------------------- the host route of the contract
def host_set_full(ests, sources, pps):
    """the contract's lio_map_set_full_cloud for every window that takes one (push form: a processor given and the full cloud on)"""
    for w, e in enumerate(ests):
        if pps is not None and pps[w] is not None and e.full_on:
            e.map().set_full_cloud(host_full(sources[w], pps[w]))


def host_items(sources, k, T=None):
    items = []
    for s in sources:
        corner, surf = host_clouds(s)
        items.append((epc.ident_T() if T is None else T, surf, corner, stamp(k)))
    return items


def host_push_batch(batch, sources, pps, k):
    """twin windows in a batch of their own: lio_est_batch_push_frames with host pointers"""
    host_set_full(batch.members, sources, pps)
    batch.push_frames(host_items(sources, k))


def host_push_single(ests, sources, pps, k):
    host_set_full(ests, sources, pps)
    for e, it in zip(ests, host_items(sources, k)):
        epc.push_single(e, it)


def host_compact(ests, sources, pps, k):
    """lio_compact_encode -> lio_est_process_compact on single handles (device_solve = 1) -> (transform_to_init per window, reports)"""
    Ts, reps = [], []
    for w, e in enumerate(ests):
        corner, surf = host_clouds(sources[w])
        full = host_full(sources[w], pps[w]) if pps is not None and pps[w] is not None else EMPTY
        T, rep = e.process_compact(e.lib.compact_encode(sources[w].T_sum(), corner, surf, full), stamp(k))
        Ts.append(T)
        reps.append(rep)
    return Ts, reps


# ---------------------------------------------------------------- the calls under test
def fed_push(batch, sources, pps, k):
    n = len(batch.members)
    before = snapshot(sources, pps or [])
    batch.push_frames_from_odom([s.od for s in sources], pps, [epc.ident_T()] * n, [stamp(k)] * n)
    assert_sources_unchanged(before, snapshot(sources, pps or []), f"push from odom, frame {k}")
    return batch.push_stats(), batch.from_odom_stats()


def fed_compact(batch, sources, pps, k):
    n = len(batch.members)
    before = snapshot(sources, pps or [])
    Ts, reps = batch.process_compact_from_odom([s.od for s in sources], pps, [stamp(k)] * n)
    assert_sources_unchanged(before, snapshot(sources, pps or []), f"compact from odom, frame {k}")
    return Ts, reps, batch.push_stats(), batch.from_odom_stats()


def refresh_both(A, B, what):
    """lio_est_refresh_map on twin windows with the map refresh on -> the record of B's (slot 0 of the ring: its corner and surf clouds), equal to A's"""
    out = []
    for w, (a, b) in enumerate(zip(A, B)):
        ra, rb = a.refresh_map(), b.refresh_map()
        assert ra == rb, (what, w, ra, rb)
        ha, hb = a.last_map_refresh(), b.last_map_refresh()
        assert ha is not None and hb is not None, (what, w)
        for key in ("corner", "surf"):
            assert ha[key].shape == hb[key].shape and np.array_equal(epc.bits(ha[key]), epc.bits(hb[key])), (what, w, key)
        out.append(hb)
    return out


def assert_same_T(Ta, Tb, what):
    for w, (a, b) in enumerate(zip(Ta, Tb)):
        assert np.array_equal(mfo.bits(a), mfo.bits(b)), (what, "transform_to_init", w)


def window(hip, W, Wo, seed, full=False, **kw):
    e = epc.window(hip, W, Wo, seed, full=full, **kw)
    e.full_on = full
    return e


def packer(hip, corner, surf, k=4):
    """a disabled odometry (the clouds stay as they are) that holds `corner` / `surf` as its last clouds"""
    s = Source(hip, prep=(k,), enabled=False)
    s.crafted(corner, surf)
    return s

