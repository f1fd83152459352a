"""The per-ring feature picks of the reference, stated serially in numpy fp32 (src/point_processor/PointProcessor.cc): PrepareRing
:542-585, the subregion bounds :672-675 (a subregion with ep <= sp is skipped, :678), PrepareSubregion :587-622, the pick loops
:685-732 with MaskPickedInRing :624-645, the per-ring voxel filter with the rel-time recompute :737-778, and the ring split of the
ring-field overload :428-536.  Every fp32 operation is rounded to np.float32 in the reference's order: squared norms are
(x*x + y*y) + z*z, the curvature sum is d += (p[i+t] + p[i-t]), and the comparisons against 0.1, 0.05 and 0.0002 * dis2 are made in
double, as the reference's literals make them.  The forward fill of PrepareRing at i = n - nc - 1 stops at the ring's end (the
reference writes one element past its vector there).

This is the contract that tests/test_ring_pick.py holds the oracle to and tests/test_gpu_ring_pick.py the product's k_ring_pick,
k_lf_ring and k_pp_pack.  Besides the results it returns counters of what a ring exercised, to which tests/ring_pick_cases.py is
held, and `plant=` switches one deliberate error on (PLANTS): every one of them must change the outcome of at least one case.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from second_source import voxel_grid_pcl  # noqa: E402

F = np.float32
TWO_PI = 2 * np.pi

DEFAULTS = dict(scan_period=0.1, num_scan_subregions=8, num_curvature_regions=5, surf_curv_th=0.1, max_corner_sharp=2,
                max_corner_less_sharp=20, max_surf_flat=4, less_flat_filter_size=0.2)

PLANTS = ("zone_blind",               # a subregion does not see what its predecessors' picks reach
          "reach_ignores_gaps",       # MaskPickedInRing does not stop at a step above 0.05 m^2
          "ties_high_index_first",    # equal curvatures sorted by descending index
          "threshold_inclusive",      # >= / <= surf_curv_th
          "one_point_subregions",     # ep == sp processed
          "prepare_fill_nc",          # PrepareRing fills nc instead of nc + 1
          "sharp_quota_per_ring",     # max_corner_sharp counted per ring instead of per subregion
          "less_sharp_in_less_flat")  # label <= 1 goes to the voxel filter


def config(over=None):
    c = dict(DEFAULTS)
    c.update(over or {})
    return c


def _sq(d):
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def subregion_bounds(n, ns, nc):
    """[(sp, ep)] per subregion, :672-675 (size_t arithmetic; ep >= sp - 1 always, so nothing wraps for n > 2 nc + 1)"""
    return [((nc * (ns - j) + (n - nc) * j) // ns, (nc * (ns - 1 - j) + (n - nc) * (j + 1)) // ns - 1) for j in range(ns)]


def prepare_ring(p, nc, plant=None, counters=None):
    """:542-585 -> mask (uint8)"""
    n = len(p)
    m = np.zeros(n, np.uint8)
    fill = nc if plant == "prepare_fill_nc" else nc + 1
    idx = np.arange(nc, n - nc)
    diff_next2 = _sq(p[idx] - p[idx + 1])
    diff_prev2 = _sq(p[idx] - p[idx - 1])
    dis2 = _sq(p[idx])
    done = np.zeros(len(idx), bool)
    for k in np.flatnonzero(diff_next2.astype(np.float64) > 0.1):
        i = int(idx[k])
        pc, pn = p[i], p[i + 1]
        depth, depth_next = np.sqrt(_sq(pc)), np.sqrt(_sq(pn))
        if depth > depth_next:
            wd = np.sqrt(_sq(pn - pc * F(depth_next / depth))) / depth_next
            if float(wd) < 0.1:
                m[i - nc:i - nc + fill] = 1
                done[k] = True
                if counters is not None:
                    counters["prepare_closer"] += 1
        else:
            wd = np.sqrt(_sq(pc - pn * F(depth / depth_next))) / depth
            if float(wd) < 0.1:
                m[i + 1:min(i + 1 + fill, n)] = 1
                done[k] = True
                if counters is not None:
                    counters["prepare_farther"] += 1
    lim = 0.0002 * dis2.astype(np.float64)
    par = ~done & (diff_next2.astype(np.float64) > lim) & (diff_prev2.astype(np.float64) > lim)
    m[idx[par]] = 1
    if counters is not None:
        counters["prepare_parallel"] += int(par.sum())
    return m


def curvature(p, sp, ep, nc):
    """:598-609 for i in [sp, ep]"""
    i = np.arange(sp, ep + 1)
    d = F(-2 * nc) * p[i]
    for t in range(1, nc + 1):
        d = d + (p[i + t] + p[i - t])
    return _sq(d)


def ring_picks(xyz, cfg=None, plant=None):
    """One ring (n x 3 float32, ring order) -> dict: sharp / less_sharp / flat (in-ring indices in pick order), mask, curvature,
    label (2 / 1 / 0 / -1; 127 outside every processed subregion), members (in-ring indices handed to the voxel filter), counters."""
    cfg = config(cfg)
    assert plant is None or plant in PLANTS
    p = np.ascontiguousarray(xyz, F).reshape(-1, 3)
    n = len(p)
    nc, ns = cfg["num_curvature_regions"], cfg["num_scan_subregions"]
    th = F(cfg["surf_curv_th"])
    counters = dict(zone_picked={}, zone_decisive={}, ties=0, sizes=[], exhausted=0, cut_forward=0, cut_backward=0, spans_subregion=0,
                    prepare_closer=0, prepare_farther=0, prepare_parallel=0, at_threshold=0, no_pick_loops=0)
    out = dict(sharp=[], less_sharp=[], flat=[], mask=np.zeros(n, np.int32), curvature=np.zeros(n, F), label=np.full(n, 127, np.int8),
               members=np.zeros(0, np.int64), counters=counters)
    if n <= 2 * nc + 1:                                   # :660 on scan_ranges = (first, last)
        return out
    m = prepare_ring(p, nc, plant, counters)
    prep = m.copy()
    gap = _sq(p[1:] - p[:-1]).astype(np.float64) > 0.05   # step i -> i + 1
    if plant == "reach_ignores_gaps":
        gap[:] = False
    bounds = subregion_bounds(n, ns, nc)
    label, curv = out["label"], out["curvature"]
    ring_sharp = 0

    def mask_picked(idx, masks):
        nf = nb = nc
        for q in range(1, nc + 1):
            if gap[idx + q - 1]:
                nf = q - 1
                break
        for q in range(1, nc + 1):
            if gap[idx - q]:
                nb = q - 1
                break
        counters["cut_forward"] += nf < nc
        counters["cut_backward"] += nb < nc
        for mm in masks:
            mm[idx - nb:idx + nf + 1] = 1
        return nf

    for j, (sp, ep) in enumerate(bounds):
        counters["sizes"].append(ep - sp + 1)
        if ep < sp or (ep == sp and plant != "one_point_subregions"):
            continue
        c = curvature(p, sp, ep, nc)
        curv[sp:ep + 1] = c
        label[sp:ep + 1] = 0
        ids = np.arange(sp, ep + 1)
        order = np.lexsort((-ids if plant == "ties_high_index_first" else ids, c))   # std::sort of pair<float, size_t>
        cs, is_ = c[order], ids[order]
        counters["ties"] += int((cs[1:] == cs[:-1]).sum())
        counters["at_threshold"] += int((cs == th).sum())
        local = prep.copy()                               # what this subregion would see without its predecessors' picks
        see = local if plant == "zone_blind" else m
        masks = (m, local)

        def decide(idx, passes):
            """-> pick it?  Counts the decisions taken in the subregion's first nc points."""
            if not passes:
                return False
            zone = j > 0 and idx < sp + nc
            if see[idx]:
                if zone and m[idx] and not local[idx]:
                    counters["zone_decisive"][j] = counters["zone_decisive"].get(j, 0) + 1
                return False
            if zone:
                counters["zone_picked"][j] = counters["zone_picked"].get(j, 0) + 1
            return True

        def picked(idx):
            nf = mask_picked(idx, masks)
            nxt = [b for b in bounds[j + 1:] if b[1] > b[0]]
            if nxt and idx + nf >= nxt[0][1] and nxt[0][0] > ep:
                counters["spans_subregion"] += 1          # the reach covers the whole next processed subregion

        num, k, picks_here = 0, len(is_), 0
        while k > 0 and num < cfg["max_corner_less_sharp"]:
            k -= 1
            idx, cv = int(is_[k]), cs[k]
            if decide(idx, cv >= th if plant == "threshold_inclusive" else cv > th):
                num += 1
                sharp = (ring_sharp < cfg["max_corner_sharp"]) if plant == "sharp_quota_per_ring" else (num <= cfg["max_corner_sharp"])
                if sharp:
                    label[idx] = 2
                    out["sharp"].append(idx)
                    ring_sharp += 1
                else:
                    label[idx] = 1
                out["less_sharp"].append(idx)
                picked(idx)
        counters["exhausted"] += num < cfg["max_corner_less_sharp"]
        picks_here += num
        num, k = 0, 0
        while k < len(is_) and num < cfg["max_surf_flat"]:
            idx, cv = int(is_[k]), cs[k]
            k += 1
            if decide(idx, cv <= th if plant == "threshold_inclusive" else cv < th):
                num += 1
                label[idx] = -1
                out["flat"].append(idx)
                picked(idx)
        counters["exhausted"] += num < cfg["max_surf_flat"]
        picks_here += num
        counters["no_pick_loops"] += picks_here == 0
    out["mask"] = m.astype(np.int32)
    out["members"] = np.flatnonzero(label <= (1 if plant == "less_sharp_in_less_flat" else 0))
    return out


def azimuth(x, y):
    """float(2 pi - atan2f(y, x)), folded below 2 pi (:462-466)"""
    a = (TWO_PI - np.arctan2(y.astype(F), x.astype(F)).astype(np.float64)).astype(F)
    return np.where(a.astype(np.float64) >= TWO_PI, (a.astype(np.float64) - TWO_PI).astype(F), a)


def ring_split(scan, ring, rings, scan_period=0.1):
    """PointToRing(PointIR) :428-536 -> (offsets [rings + 1], ring cloud [N x 4, intensity = ring + rel_time], source index per point,
    start_ori).  Keeps the finite points whose ring lies in [0, rings), in input order per ring."""
    scan = np.ascontiguousarray(scan, F).reshape(-1, 4)
    ring = np.asarray(ring).astype(np.int64)
    keep = np.flatnonzero(np.isfinite(scan[:, :3]).all(1) & (ring >= 0) & (ring < rings))
    offsets = np.zeros(rings + 1, np.int32)
    if len(keep) == 0:
        return offsets, np.zeros((0, 4), F), keep, F(0)
    azi = azimuth(scan[keep, 0], scan[keep, 1])
    start = azi[0]
    azi = np.where(azi - start < 0, (azi.astype(np.float64) + TWO_PI).astype(F), azi)   # half_passed never sets (:488)
    end = max(F(0), azi.max())
    range_ori = F(end - start)
    rel_time = (scan_period * (azi - start).astype(np.float64) / np.float64(range_ori)).astype(F)
    order = np.argsort(ring[keep], kind="stable")
    src = keep[order]
    r_sorted = ring[src]
    offsets[1:] = np.cumsum(np.bincount(r_sorted, minlength=rings))
    cloud = scan[src].copy()
    cloud[:, 3] = r_sorted.astype(F) + rel_time[order]
    return offsets, cloud, src, start


def less_flat_of_ring(ring_cloud, members, leaf, start_ori, scan_period=0.1):
    """:737-778 for one ring: VoxelGrid over the members in ring order, then intensity = int(centroid intensity) + rel_time of the
    centroid's azimuth against start_ori."""
    if len(members) == 0:
        return np.zeros((0, 4), F)
    c, _ = voxel_grid_pcl(ring_cloud[members], leaf)
    rel = azimuth(c[:, 0], c[:, 1]) - F(start_ori)
    rel = np.where(rel < 0, (rel.astype(np.float64) + TWO_PI).astype(F), rel)
    rel_time = (scan_period * rel.astype(np.float64) / TWO_PI).astype(F)
    c[:, 3] = np.trunc(c[:, 3]).astype(F) + rel_time
    return c


def sweep_reference(scan, ring, rings, cfg=None, plant=None):
    """A whole sweep through the ring-field overload -> dict with offsets, ring_cloud, start_ori, per class (ring, idx) lists and
    clouds in the reference's order (ring by ring, subregion by subregion), mask, curvature, less_flat, and the rings' counters."""
    cfg = config(cfg)
    offsets, cloud, _, start = ring_split(scan, ring, rings, cfg["scan_period"])
    res = dict(offsets=offsets, ring_cloud=cloud, start_ori=float(start), mask=np.zeros(len(cloud), np.int32), curvature=np.zeros(len(cloud), F),
               counters=[], members=[])
    lists = {k: ([], []) for k in ("sharp", "less_sharp", "flat")}
    lf = []
    for r in range(rings):
        a, e = int(offsets[r]), int(offsets[r + 1])
        rp = ring_picks(cloud[a:e, :3], cfg, plant)
        res["mask"][a:e], res["curvature"][a:e] = rp["mask"], rp["curvature"]
        res["counters"].append(rp["counters"])
        res["members"].append(len(rp["members"]))
        for k in lists:
            lists[k][0].extend([r] * len(rp[k]))
            lists[k][1].extend(rp[k])
        lf.append(less_flat_of_ring(cloud[a:e], rp["members"], cfg["less_flat_filter_size"], start, cfg["scan_period"]))
    for k, (rr, ii) in lists.items():
        rr, ii = np.asarray(rr, np.int32), np.asarray(ii, np.int32)
        res[k] = (rr, ii)
        res[k + "_cloud"] = cloud[offsets[rr] + ii] if len(rr) else np.zeros((0, 4), F)
    res["less_flat"] = np.concatenate(lf) if lf else np.zeros((0, 4), F)
    return res
