// batch_kernels.h — the map / feature stages of Estimator::SolveOptimization for B windows at once:
// every stage of BuildLocalMap (Estimator.cc:1361-1646), CalculateFeatures (:970-1097) and CalculateLaserOdom (:1242-1359) is
// ONE launch over all windows of the batch, indexed by blockIdx.y / .z through a per-window descriptor in device memory.
// The per-window arithmetic is the single-window kernels' (cloud_device.h), and every partition (blocks of a round, tiles of a
// filter) is a function of the window's own sizes: a window gives the same bits alone (B = 1) and inside any batch.
// The local maps' voxel filter behind the concat is the segmented filter of seg_vox.h, which the batched push (est_push.h) runs too.
#pragma once
#include "cloud_kernels.h"
#include "seg_sort.h"
#include "seg_vox.h"

namespace lio {

#define LIO_BW_MAX_SEG 8        // segments of a local map: the pivot's cloud + the Wo - 1 frames behind it (Wo <= 7)
#define BW_KEY_NONE 0x7FFFFFFFu  // stored voxel key of the batched filter (absolute cells, 31 bits): all ones = no point
#define LIO_BW_MAX_STATIC 7     // frames whose features do not depend on the newest frame's rounds

struct BatchWin {
  // ---- BuildLocalMap: concat into local_all[vox.off, vox.off + vox.n), keys, filter (vox.dst null: the batch's filtered array); vox.off is
  // this window's first point in every point array of the batch
  ConcatSeg seg[LIO_BW_MAX_SEG];
  int nseg;
  VoxSeg vox;
  // ---- feature slots: this window's range of the batch's slot arrays (valid / coef / score)
  int slot_base, n_slots;
  FeatFrame fr[LIO_BW_MAX_STATIC];   // slot_off is an offset into the batch's arrays, tf_index an index into tf
  int nstatic;
  FeatFrame newest;              // the frame CalculateLaserOdom iterates on (M = 0: none)
  int nb_round, part_off, keep;  // its search blocks per round, its first row of the batch's partials, keep_features
  float tf[LIO_BW_MAX_STATIC + 1][8];   // local transforms (qx qy qz qw px py pz pad); the last entry is the newest frame's start
  float min_match_sq_dis, min_plane_dis;
};

// the K-NN grid of a window (host-computed from the filter's bounds, uploaded before the cell build)
struct BatchGrid { GridDesc g; int cell_off; int n_filtered; };

// Execution choices of a batch that the results do NOT depend on (every one of them keeps the sums' orders): 0 = by the size of the
// launch.  They live in the batch handle (lio_est_batch_set_option).
struct BatchKnobs {
  int lanes_per_query = 0;   // 1 / 4 / 8 lanes per query of the search kernels; by size: 1 from 100 k queries, 4 from 15 k, else 8
  int loop_groups = 0;       // 1 .. 4 launch chains of the trust-region loop side by side; by size: 4 from 32 windows, 2 from 256
  int aux_threads = 0;       // 64 / 128 / 256 threads per block of the aux row; by size: 64 from 128 windows per launch
  int finish_threads = 0;    // 1 .. 8 host threads of the write-back; by size: 4 from 128 windows
  int time_kernels = 0;      // 1: HIP events around every launch of the trust-region loop's three kernels on the stream they run on (measurement
                             //    runs only: the events serialise the host's enqueue; BatchClock::kernel_ms / kernel_launches)
};

int bw_round_blocks(int M);   // search blocks of one round of a window's newest frame: 64 queries each, whatever the lanes per query

// concat + voxel keys (absolute cells) + per-block bounds: the producer in front of SegVoxFilter::finish (seg_vox.h).  keys, partial, flag: the
// filter's (keys: loc-array sized; partial: 8 floats per 256-point block)
void launch_bw_concat_keys(const BatchWin *win, int B, int max_local, float4 *local_all, uint32_t *keys, float *partial, int *flag, hipStream_t s);
// feature flags cleared, the newest frames' Gauss-Newton states started
void launch_bw_setup(const BatchWin *win, int B, int max_slots, uint8_t *valid_all, OdomState *odom, int *n_converged, hipStream_t s);
// K-NN grid: cell keys of the filtered points; (segmented sort by the caller); cell-sorted points + the dense table of run starts
void launch_bw_cell_keys(const BatchWin *win, const BatchGrid *grid, int B, int max_filtered, const float4 *filtered_all, uint32_t *keys, hipStream_t s);
void launch_bw_cell_table(const BatchWin *win, const BatchGrid *grid, int B, int max_filtered, const float4 *filtered_all, const uint32_t *keys_sorted,
                          const uint32_t *vals_sorted, int *cells_all, float4 *sorted_all, hipStream_t s);
// total_queries: stack points of the launch over all windows — picks the lanes per query (the results do not depend on it)
void launch_bw_features(const BatchWin *win, const BatchGrid *grid, int B, int max_M, int max_static, long long total_queries, const BatchKnobs &knobs,
                        const float4 *sorted_all, const int *cells_all, uint8_t *valid_all, float4 *coef_all, float *score_all, hipStream_t s);
void launch_bw_odom_round(const BatchWin *win, const BatchGrid *grid, int B, int max_nb, long long total_queries, const BatchKnobs &knobs, int round, OdomState *odom,
                          const float4 *sorted_all, const int *cells_all, uint8_t *valid_all, float4 *coef_all, float *score_all, double *partials,
                          int *n_converged, hipStream_t s);

}  // namespace lio
