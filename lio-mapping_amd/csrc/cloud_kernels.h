// cloud_kernels.h — device-side point-cloud stages of the estimator (host-callable launchers).
//   rigid transform / concat    : pcl::transformPointCloud call sites Estimator.cc:1425,1498,2602
//   VoxelGridDev                : pcl::VoxelGrid<PointXYZI> call sites Estimator.cc:678-687,1518-1519
//   KnnGrid + feature kernels   : pcl::KdTreeFLANN + Estimator::CalculateFeatures (Estimator.cc:970-1097)
//   laser-odom rows/update      : Estimator::CalculateLaserOdom (Estimator.cc:1242-1359)
//   deskew                      : TransformToEnd (Estimator.cc:62-103)
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "dev.h"
#include "hmath.h"

namespace lio {

struct VoxParams {
  float mn[3], mx[3];
  int minb[3], divb[3];
  int overflow;  // PCL's "leaf size too small" guard: output = input
  int n_valid;
};

struct Affine3f { float m[12]; };  // row-major 3x4: [R | t]

#define LIO_MAX_FRAMES 32

// dst[seg.dst_off + k] = tf * src[k] (or src[k] when identity); intensity optionally overwritten.  One segment record for the concat of one
// window (ConcatArgs), of a batch's local maps (batch_kernels.h: BatchWin) and of a batch's slides (est_push.h: BpSlide)
struct ConcatSeg { const float4 *src; int n; int dst_off; int identity; int set_intensity; float intensity; Affine3f tf; };
struct ConcatArgs { ConcatSeg seg[LIO_MAX_FRAMES]; int nseg; int total; };
void launch_transform_concat(const ConcatArgs &a, float4 *dst, hipStream_t s);

// TransformToEnd (Estimator.cc:62-103) in place; tes = q(xyzw), p.  keep_intensity (:79): the form SolveOptimization runs on the
// full-resolution cloud (:2355-2420); x y z are the same bits in both forms
void launch_deskew_to_end(float4 *pts, int n, const float q[4], const float p[3], float time_factor, hipStream_t s, bool keep_intensity = false);
// out = rot * in + pos, intensity kept (PointAssociateToMap, PointMapping.cc:303-314); out of place
void launch_rigid_map(const float4 *in, int n, const float q[4], const float p[3], float4 *out, hipStream_t s);

// The bounds pass (VoxParams) of device clouds, side by side.  A cloud of n points is reduced by cloud_bounds_blocks(n) blocks of 256 threads into
// rows of eight floats (cloud_device.h: cloud_bounds_block), which one more block folds (vox_fold_bounds).  Minimum and maximum do not hang
// on the order and the count is a float sum of integers below 2^24, so a cloud has the same VoxParams alone and in any batch.
inline int cloud_bounds_blocks(int n) { return std::max(1, std::min(cdiv(n, 256), 512)); }
struct BoundsSeg { const float4 *pts; int n, nb, off; };   // a cloud, its blocks, its first row of `partial`
// d_segs: nseg records on the device; grid (max_nb, nseg), the blocks beyond a cloud's nb leave at once; d_out[k] = cloud k's.  No host sync.
void launch_seg_bounds(const BoundsSeg *d_segs, int nseg, int max_nb, float *partial, float inv_leaf, VoxParams *d_out, hipStream_t s);

// The filter's sort of the n (key, index) pairs: a sample sort in three launches (splitters, bucket scatter, bucket sort + compaction).
// Sizing, a pure function of n:
//   n <= VSORT_CAP                      keys_ sorted directly in one launch, by rank: every workgroup holds all keys in LDS and places 16 of them
//   VSORT_CAP < n <= VSORT_MAX_N        NB = ceil(n / VSORT_MEAN) buckets of VSORT_CAP pairs each (more than 10 x the mean bucket, which is <= VSORT_MEAN;
//                                       the fullest bucket sets the third kernel's time, so the mean is small),
//                                       S = VSORT_OVERSAMPLE * NB sample keys at the positions floor((j + 0.5) n / S) of this call's keys
//   n > VSORT_MAX_N                     the library's radix sort
// A bucket that would pass its capacity raises the overflow word; finish() then redoes the filter with the library's sort.
#define VSORT_CAP 4096            // pairs a bucket holds = pairs one workgroup sorts (16 per thread; 32 KB of LDS for the strides that cross waves)
#define VSORT_MEAN 384
#define VSORT_OVERSAMPLE 8
#define VSORT_MAX_BUCKETS 1024    // splitters and per-workgroup bucket counters live in LDS
#define VSORT_MAX_N (VSORT_MAX_BUCKETS * VSORT_MEAN)
enum VoxSortPath { VSORT_PATH_SAMPLE = 0, VSORT_PATH_SINGLE = 1, VSORT_PATH_LIBRARY = 2 };
inline int vsort_buckets(size_t n) { return int((n + VSORT_MEAN - 1) / VSORT_MEAN); }

class VoxelGridDev {
 public:
  // runs whose result came from the sample sort, from the direct one-launch sort, and from the library's sort (VoxSortPath order)
  void sort_stats(unsigned long long out[3]) const { for (int k = 0; k < 3; ++k) out[k] = n_path_[k]; }
  // the sort enqueue() runs, on caller-given host keys with values = positions (lio_vox_sort_pairs); returns the path that gave the result
  int sort_pairs_hook(const uint32_t *keys, size_t n, uint32_t *keys_out, uint32_t *vals_out, hipStream_t s);
  // Filters `in` (device, n points) with cubic leaf; result in `out`; returns the output count (host sync).
  // host_params (optional) receives the bounds used.
  size_t run(const float4 *in, size_t n, float leaf, DBuf<float4> &out, hipStream_t s, VoxParams *host_params = nullptr);
  // the same in two halves: launch() only enqueues; finish() returns the count as soon as the device has posted it — the
  // centroids themselves may still be in flight on `s`, so consumers on OTHER streams must wait for `s` through an event
  void launch(const float4 *in, size_t n, float leaf, DBuf<float4> &out, hipStream_t s);
  size_t finish(VoxParams *host_params = nullptr);
  void set_host_signal(bool on) { use_signal_ = on; }   // false: counts come back by copy + hipStreamSynchronize (lio_est_config.stream_sync)
  VoxelGridDev() = default;
  VoxelGridDev(const VoxelGridDev &) = delete;
  VoxelGridDev &operator=(const VoxelGridDev &) = delete;

 private:
  const float4 *p_in_ = nullptr; size_t p_n_ = 0; DBuf<float4> *p_out_ = nullptr; hipStream_t p_stream_ = nullptr;  // the pending launch
  float p_leaf_ = 0.f;
  void enqueue(bool exact, bool library);
  void reserve_sort(size_t n, hipStream_t s);
  int enqueue_sort(size_t n, hipStream_t s, bool library);   // keys_ / vals_ -> keys2_ / vals2_; returns the VoxSortPath taken
  DBuf<uint32_t> splitters_;
  DBuf<int> fill_;
  DBuf<unsigned long long> pairs_;  // NB bucket regions of VSORT_CAP pairs (key << 32 | index)
  int last_path_ = VSORT_PATH_LIBRARY;
  unsigned long long n_path_[3] = {0, 0, 0};
  HostBuf<char> h_mail_;           // pinned, coherent, allocated on first use
  int *h_count_ = nullptr;          // ... its views: output count, followed by the VoxParams
  VoxParams *h_params_ = nullptr;
  DBuf<float> partial_;
  DBuf<VoxParams> params_;
  DBuf<uint32_t> keys_, keys2_, vals_, vals2_;
  DBuf<int> count_, tile_heads_;
  DBuf<char> tmp_;
  unsigned *h_flag_ = nullptr;      // completion word behind the mailbox (dev.h: HostSignal)
  unsigned seq_ = 0;
  HostSignal sig_{};
  bool use_signal_ = true;
};

struct GridDesc {
  int origin[3];   // cell coordinate of cell (0,0,0)
  int dims[3];
  float inv_cell;
  int n_points;
};

// Cell edge >= sqrt(min_match_sq_dis): the 27-cell neighbourhood then holds every point that can pass the d2[4] < min_match_sq_dis
// gate (Estimator.cc:1021).  odometry.hip sizes its grids by an expression of its own.
inline float knn_cell_edge(float min_match_sq_dis) { return std::sqrt(min_match_sq_dis) * 1.0001f + 1e-6f; }
// ... and the edge the scan-to-map grids (mapping.hip, kf_batch.hip) have always had: no + 1e-6f, so a different partition of the same points
inline float scan_to_map_cell_edge(float min_match_sq_dis) { return std::sqrt(min_match_sq_dis) * 1.0001f; }
// min / max of the points of a host cloud (x y z i) that are finite in x, y and z; zeros when there is none
inline void host_cloud_bounds(const float *xyzi, size_t n, float mn[3], float mx[3]) {
  for (int d = 0; d < 3; ++d) { mn[d] = 0.f; mx[d] = 0.f; }
  bool first = true;
  for (size_t i = 0; i < n; ++i) {
    const float *p = xyzi + 4 * i;
    if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2])) continue;
    for (int d = 0; d < 3; ++d) {
      if (first || p[d] < mn[d]) mn[d] = p[d];
      if (first || p[d] > mx[d]) mx[d] = p[d];
    }
    first = false;
  }
}
// inv_cell, origin, dims of the grid over [mn, mx] with one border cell on every side; returns the number of cells
inline size_t grid_extent(GridDesc &g, const float mn[3], const float mx[3], float cell) {
  g.inv_cell = 1.0f / cell;
  size_t ncells = 1;
  for (int d = 0; d < 3; ++d) {
    const int lo = int(std::floor(mn[d] * g.inv_cell)) - 1, hi = int(std::floor(mx[d] * g.inv_cell)) + 1;
    g.origin[d] = lo; g.dims[d] = hi - lo + 1;
    ncells *= size_t(g.dims[d]);
  }
  return ncells;
}

class KnnGrid {
 public:
  // Uniform grid over `pts` (device, n points).  bounds = min/max of the region to index (host values); points
  // outside it are clamped into the border cells (still compared by true distance).
  void build(const float4 *pts, size_t n, const float mn[3], const float mx[3], float cell, hipStream_t s);
  const float4 *sorted() const { return sorted_.p; }   // xyz + original index in .w (int bits)
  const int *cells() const { return cells_.p; }         // ncells + 1 run starts: cell c holds sorted()[cells[c] .. cells[c + 1])
  const GridDesc &desc() const { return desc_; }

 private:
  GridDesc desc_{};
  DBuf<uint32_t> keys_, keys2_, vals_, vals2_;
  DBuf<float4> sorted_;
  DBuf<int> cells_, cnt_;
  // The count table's invariant (GridBatch's too): all zeros between builds.  A fresh table is filled once; after that every point's place
  // kernel puts its cell's count back, so a build needs no fill command.  dirty: a count kernel was enqueued and its place kernel was not (a
  // build that threw in between) — the next build fills the table again.
  bool cnt_dirty_ = false;
  DBuf<char> tmp_;
};

// The grids of a call's clouds, built side by side: the bounds pass above over all of them (two launches, one read-back, one wait), the layout
// on the host, then KnnGrid::build's counting sort (cell_count_point, block_exclusive_scan, cell_place_point) in three launches over all of
// them.  Every grid has its slice of one count table and one cell table, and its run starts are offsets into ONE sorted array.  The records the
// kernels read lie behind the caller's own records (`head`) in one staging table: the bounds pass uploads the BoundsSeg records alone, the
// build the head and the GridSeg records in one copy.
struct GridSeg { const float4 *pts; GridDesc g; int pt_off, cell_off, ncells; };   // pt_off < 0: not built here
class GridBatch {
 public:
  // a call: room for head_bytes (a multiple of 8) of the caller's records and for `clouds` clouds; returns the caller's part, zeroed
  void *begin(size_t head_bytes, int clouds);
  const void *head_dev() const { return d_tab_.p; }
  void add(const float4 *pts, int n);
  // upload of the clouds' BoundsSeg records, the two launches, one read-back, one wait: cloud i's bounds at [i]
  const VoxParams *bounds(hipStream_t s, float inv_leaf = 1.0f);
  // the grids over the bounds (a cloud without a finite point: over the origin) at the given cell edge, and their slices; a grid of more than
  // cells_cap cells gets none (shared(i) false: the caller builds it with a KnnGrid of its own, with desc(i))
  void layout(float cell, size_t cells_cap);
  bool shared(int i) const { return gseg(i).pt_off >= 0; }
  const GridDesc &desc(int i) const { return gseg(i).g; }
  const float4 *sorted(int) const { return sorted_.p; }
  const int *cells(int i) const { return cells_.p + gseg(i).cell_off; }
  // upload of the head as the caller left it and the GridSeg records, then count, scan and place of the shared grids
  void build(hipStream_t s);

 private:
  BoundsSeg *bseg() { return reinterpret_cast<BoundsSeg *>(h_tab_.data() + off_b_); }
  GridSeg &gseg(int i) const { return reinterpret_cast<GridSeg *>(const_cast<char *>(h_tab_.data()) + off_g_)[i]; }
  std::vector<char> h_tab_;   // head | GridSeg x clouds | BoundsSeg x clouds
  DBuf<char> d_tab_;
  size_t off_b_ = 0, off_g_ = 0, part_total_ = 0;
  int n_ = 0, max_nb_ = 0, max_pts_ = 0;
  bool any_shared_ = false;
  DBuf<float> partial_;
  DBuf<VoxParams> d_bounds_;
  HostBuf<VoxParams> h_bounds_;   // pinned landing zone
  DBuf<uint32_t> keys_, slot_;
  DBuf<int> cnt_, cells_;
  DBuf<float4> sorted_;
  bool cnt_dirty_ = false;        // (KnnGrid: the count table's invariant)
};

// order (optional): the queries are PROCESSED in this order — order[t] = slot (slot_off + index into stack) of the t-th query — so that the lanes
// of a wave search neighbouring map cells and their gathers fall into the same cache lines; results go to the queries' own slots, so nothing
// downstream sees the order
struct FeatFrame { const float4 *stack; int M; int slot_off; int tf_index; const uint32_t *order = nullptr; };
struct FeatArgs {
  FeatFrame fr[LIO_MAX_FRAMES];
  int nframes;
  int max_M;
  float min_match_sq_dis, min_plane_dis;
  // 0 in every launch that takes a FeatArgs (the estimator's); the scan-to-map forms (1 PointMapping, 2 MapBuilder::OptimizeMap) reach the
  // shared bodies as FeatScalars from the keyframe kernels below.  Both fields stay: they are part of these kernels' argument layout.
  int mapping_mode;
  float fixed_pz[3];
};
// transforms: device array of 8 floats per entry (qx,qy,qz,qw,px,py,pz,pad).  skip_flag: optional device int;
// when *skip_flag != 0 the launch is a no-op (converged laser-odom loop).
void launch_features(const FeatArgs &a, const float *transforms, const float4 *map_sorted, const int *cells, const GridDesc &g,
                     uint8_t *valid, float4 *coef, float *score, const int *skip_flag, hipStream_t s);

// stateless K-NN (lio_knn entry point): the product's walk (knn_scan_group, 8 lanes per query), k = 1 or 5, entries at or beyond
// radius_sq come back as -1 / +inf; idx / sqd are m * k
void launch_knn(const float4 *query, int m, int k, float radius_sq, const float4 *map_sorted, const int *cells, const GridDesc &g,
                int32_t *idx, float *sqd, hipStream_t s);
// the same walk with 1, 4 or 8 lanes per query and no radius cut (lio_knn_walk, include/lio_test_hooks.h): idx / sqd are m * 5,
// nbr_xyz (m * 5 * 3) the coordinates at the positions the walk hands to the plane fit
void launch_knn_walk(const float4 *query, int m, int lanes_per_query, const float4 *map_sorted, const int *cells, const GridDesc &g,
                     int32_t *idx, float *sqd, float *nbr_xyz, hipStream_t s);

// the plane fit (form 0 estimator, 1 PointMapping, 2 MapBuilder) or the line fit (form 3) of the product on caller-given neighbours, one
// query per lane (lio_fit_five, include/lio_test_hooks.h): nbr is m * 5 points, fifth_sqd m; every output is m entries, zeros where invalid
void launch_fit_five(int form, float min_match_sq_dis, float min_plane_dis, const float fixed_pz[3], const float *transform, const float4 *stack,
                     int m, const float4 *nbr, const float *fifth_sqd, uint8_t *valid, float4 *coef, float *score, float4 *abs_coef, hipStream_t s);

// What a solve's feature stage starts from, in ONE launch instead of a fill and two small uploads (each a command of its own in
// the stream, the uploads staged through the runtime's pinned buffer): valid[0, n_valid) <- 0, the (W + 1) x 8 local transforms,
// the newest frame's Gauss-Newton state.
struct SolveSetup {
  float tf[LIO_MAX_FRAMES][8];
  int ntf;
  float odom_T[8];
  int set_odom;
};
struct OdomState;
void launch_solve_setup(const SolveSetup &a, float *d_transforms, OdomState *d_odom, uint8_t *valid, size_t n_valid, hipStream_t s);

struct OdomState {
  float T[8];        // qx,qy,qz,qw,px,py,pz,pad : local_transform of the newest frame
  int converged;
  int iters;
  int degenerate;
  int kz;            // number of leading components masked (A.6)
  int nsel;          // rows selected in the last round
};
// What the odometry's TransformToEnd runs a cloud through (OdometryDev::View, MapFullSource): the device-side transform_es_ the last step
// left, and the handle's two de-skew parameters.  st null: a copy (odometry disabled, or no publishing step yet).
struct ToEnd { const OdomState *st; float time_factor; int no_deskew; };
// The device record of a full cloud written by a take launch (mapping.hip: k_mb_from_odom's row 2; est_push.hip: k_bp_take_keys_dev's rows
// behind the clouds): lio_odom_full_to_end then lio_map_set_full_cloud with no copy between.  cloud_device.h: full_take_body.
struct FullTake { const float4 *in; float4 *out; int n; ToEnd to_end; };
// the state a Gauss-Newton loop starts from at pose T: no round run, nothing converged
inline OdomState odom_state_at(const Rigid<float> &T) {
  OdomState st{};
  st.T[0] = T.rot.x; st.T[1] = T.rot.y; st.T[2] = T.rot.z; st.T[3] = T.rot.w;
  st.T[4] = T.pos.x; st.T[5] = T.pos.y; st.T[6] = T.pos.z;
  return st;
}
// point_on_z_axis_ of a pose (PointMapping.cc:803-806): the apex of the FOV test, fixed before the scan-to-map iterations
inline void point_on_z_axis(const Rigid<float> &T, float pz[3]) {
  const Vec3<float> z = rotate(T.rot, Vec3<float>(0.f, 0.f, 10.f));
  pz[0] = z.x + T.pos.x; pz[1] = z.y + T.pos.y; pz[2] = z.z + T.pos.z;
}
// The states of n sensors posted by one launch (one block each, state_mail_slot + post_host_mail) and the completion words behind them, in
// pinned coherent memory: STATE_MAIL_STRIDE bytes per slot, then one word per slot (dev.h: HostSignal).
class StateMail {
 public:
  // room for n sensors, zeroed when it grows (by half).  Only between calls: the stream is idle, nobody still posts to the old memory
  void reserve(int n) {
    if (cap_ >= size_t(n)) return;
    cap_ = size_t(n) + size_t(n) / 2;
    buf_.alloc(cap_ * (STATE_MAIL_STRIDE + sizeof(unsigned)), hipHostMallocCoherent, true);
  }
  char *base() const { return buf_.p; }
  OdomState &slot(int j) const { return *reinterpret_cast<OdomState *>(buf_.p + size_t(j) * STATE_MAIL_STRIDE); }
  // the signal of the next launch that posts n states
  const HostSignal &arm(int n) {
    sig_.flag = reinterpret_cast<unsigned *>(buf_.p + cap_ * STATE_MAIL_STRIDE); sig_.seq = ++seq_; sig_.nslots = n;
    return sig_;
  }
  void wait(hipStream_t s) const { wait_host_signal(sig_, s); }   // for the last armed launch
  bool all_converged(int n) const {
    bool all = true;
    for (int j = 0; j < n; ++j) all = all && slot(j).converged;
    return all;
  }

 private:
  HostBuf<char> buf_;
  size_t cap_ = 0;
  unsigned seq_ = 0;
  HostSignal sig_{};
};
static_assert(sizeof(OdomState) <= STATE_MAIL_STRIDE, "mailbox layout");

// blocks of a row reduction over nslots slots (28 doubles of partials each)
int odom_rows_blocks(int nslots);
// One round of the newest frame's loop in two launches (search + plane fit + rows per block; fold + update).  a.fr[0] names the
// stack; slots of round r start at base_slot (+ r * M with keep != 0: keep_features, Estimator.cc:978-980); partials holds
// odom_round_blocks(M, lanes per query) x 28 doubles.
int odom_round_blocks(int M, int lpq);
void launch_odom_round(const FeatArgs &a, int base_slot, int round, int keep, OdomState *st, const float4 *map_sorted, const int *cells, const GridDesc &g,
                       uint8_t *valid, float4 *coef, float *score, double *partials, hipStream_t s, OdomState *mail = nullptr,
                       const HostSignal &sig = HostSignal(), int lpq = 8);

// ---- the Gauss-Newton test hooks (include/lio_test_hooks.h)
// the row of every slot on its own (7 floats: a0 .. a5, b; zeros where valid is 0), one query per lane through the row function of the rows kernels
void launch_gn_rows_map(const float4 *stack, int m, const uint8_t *valid, const float4 *coef, const OdomState *st, int b_from_coef, uint8_t *ok_out,
                        float *rows_out, hipStream_t s);
// sums_out[28] (device) = reduce_partials28 on 256 threads (wide == 0) or fold_partials28_wide on 1024
void launch_gn_fold(const double *partials, int nblocks, int wide, double *sums_out, hipStream_t s);
// odom_update_from_sums on device sums and a device state, in place
void launch_gn_step(const double *sums, OdomState *st, int iter, int min_rows, int left_update, hipStream_t s);

// ---- the scan-to-map Gauss-Newton loop (OptimizeMap / OptimizeTransformTobeMapped, MapBuilder.cc:624-1014, PointMapping.cc:325-753) for a
// table of keyframes: B independent loops in the batched refinement (config 5, kf_batch.hip), the iterating sensors of a call in the map handles
// (mapping.hip; lio_map_process: a table of one).
// Slots of keyframe k = [slot_off, slot_off + Mc) corner, then Ms surf, in one concatenated stack.  Three launches per round:
//   round  : corner line search + surf plane search (PointMapping.cc:377-619), blockIdx.y picks the branch
//   rows   : mat_A / mat_B (Estimator.cc:1272-1301) reduced to nb partials of 28 doubles.  b_from_coef != 0: mat_B = -coef.w (the distance
//            stored at feature time, PointMapping.cc:640,650); 2 additionally maps the rotation columns into the map frame with the
//            MapBuilder weights (MapBuilder.cc:903-914)
//   update : fold + 6x6 solve + degeneracy mask + transform update + convergence test (Estimator.cc:1303-1357).  min_rows > 0: a round with
//            fewer selected rows leaves the transform untouched (`continue`, PointMapping.cc:623-626).  left_update != 0: rot = DeltaQ(x) * rot
//            (MapBuilder.cc:978-979) instead of rot * DeltaQ(x)
struct KfDesc {
  int slot_off, Mc, Ms;
  int map;          // index into the KfMapDesc array
  int nb;           // row-reduction blocks of this keyframe (= odom_rows_blocks(Mc + Ms))
  int part_off;     // first partial row (28 doubles each)
  float pz[3];      // point_on_z_axis_ fixed before the iterations
};
struct KfMapDesc {
  const float4 *corner_sorted; const int *corner_cells; GridDesc corner_grid;
  const float4 *surf_sorted; const int *surf_cells; GridDesc surf_grid;
};
// grid z limit: n_keyframes <= 65535 per launch
// order_or_null: processing order of every keyframe's queries (global slots; a keyframe's corner queries at [slot_off, slot_off + Mc), its surf
// queries behind them), e.g. sorted by map cell (launch_kf_query_keys + the segmented sort)
void launch_kf_query_keys(const KfDesc *kd, const KfMapDesc *md, const OdomState *st, int n_keyframes, int max_Mc, int max_Ms, const float4 *stack_all, uint32_t *keys,
                          hipStream_t s);
// lpq: lanes per query, 1, 4 or 8 (the result does not depend on it).  abs_coef_or_null: the unsigned plane of every valid surf query at
// its slot (the map handle's score list, PointMapping.cc:572-592)
void launch_kf_round(const KfDesc *kd, const KfMapDesc *md, const OdomState *st, int n_keyframes, int max_Mc, int max_Ms, int lpq, const float4 *stack_all,
                     const uint32_t *order_or_null, float min_match_sq_dis, float min_plane_dis, int mapping_mode, uint8_t *valid, float4 *coef,
                     float4 *abs_coef_or_null, hipStream_t s);
void launch_kf_rows(const KfDesc *kd, const OdomState *st, int n_keyframes, int max_nb, const float4 *stack_all, const uint8_t *valid, const float4 *coef,
                    double *partials, int b_from_coef, hipStream_t s);
// n_converged (device int, optional) is incremented once per keyframe when it converges.  sig.flag != nullptr: behind the update block k posts
// keyframe k's state to its own slot of the host's mailbox (StateMail::base(), armed for n_keyframes) and then sig.seq to its own completion
// word, converged before this launch or not
void launch_kf_update(const KfDesc *kd, OdomState *st, int n_keyframes, const double *partials, int iter, int min_rows, int left_update, int *n_converged,
                      char *mail, const HostSignal &sig, hipStream_t s);

#if defined(__HIPCC__)
// Fixed-order sum of `nblocks` rows of 28 doubles by a 256-thread block: 8 groups of 32 lanes take the rows b = g (mod 8)
// in ascending order, then the 8 group sums are added in ascending g.  (One lane per column walking all rows issues
// ~nblocks dependent-latency loads: 18 us for 38 rows.)
__device__ inline void reduce_partials28(const double *__restrict__ partials, int nblocks, double *ssum /* shared, >= 28 */) {
  __shared__ double part28[8][32];
  const int c = threadIdx.x & 31, g = threadIdx.x >> 5;
  double v = 0;
  if (c < 28 && g < 8)
    for (int b = g; b < nblocks; b += 8) v += partials[b * 28 + c];
  if (g < 8) part28[g][c] = v;
  __syncthreads();
  if (threadIdx.x < 28) {
    double s = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) s += part28[k][threadIdx.x];
    ssum[threadIdx.x] = s;
  }
  __syncthreads();
}
#endif

}  // namespace lio
