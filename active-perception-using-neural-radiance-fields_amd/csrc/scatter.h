// Host interface of the table-gradient scatter (scatter.hip): what the field's backward (train.hip backward_impl) needs of it and nothing more.
#pragma once
#include "field.h"

namespace mnf {

// Regions of the train workspace the scatter uses for an upper bound of n samples (the caller places them): bytes of the private copies of the coarsest
// levels' gradient, and 16-byte items of the binned levels' lists (none below 8192 samples)
struct ScatterWorkspace { size_t repl_bytes, bin_items; };
ScatterWorkspace scatter_workspace(const mnf_field_s *f, int64_t n);

// List cursors of the binned levels: device uint32 the caller owns and owes the scatter ZEROED — on its own stream, in front of the first event of
// ev_chunk (train.hip: gather_fragsT_kernel clears them on a launch that runs before the fork; a memset on the bins' stream cost 335 us there).
constexpr int kScatterCursors = 16 * 512;

struct ScatterCall {
    const mnf_field_s *f;
    const float *dX;                    // [16][Np][4] un-scaled feature gradients, level-major (dgrad_kernel)
    const float *xn;                    // [n][3] aabb-normalised positions
    int64_t Np, n;
    const int64_t *n_dev;               // the sample count on the device (n = its upper bound), or NULL
    float *g_table;                     // fp32 [entries][4], added to (deterministic mode: overwritten)
    float *repl; float4 *bin_items; size_t bin_items_n;      // workspace regions (scatter_workspace)
    int n_chunks; bool deterministic;   // ranges of tiles dgrad was launched for (field_dev.h chunk_tiles); the fixed-point route
    hipStream_t stream, side, side2;    // the caller's stream (joined by the bins), the walk's, the bins'
    const hipEvent_t *ev_chunk;         // [n_chunks] recorded on `stream` behind each range's dgrad
    hipEvent_t ev_join2;                // the scatter's own: the bins' join
    unsigned long long **d_qtable;      // deterministic mode's fixed-point gradient: allocated here on first use, owned (freed) by the caller
    uint32_t *d_bin_cursors;            // [kScatterCursors]
};

// ScatterCall::xn for a caller whose forward did not leave it: (x - aabb_min) / (aabb_max - aabb_min) of n (or *n_dev) positions, one launch on `stream`
void scatter_normalize(const mnf_field_s *f, const float *positions, int64_t n, const int64_t *n_dev, float *xn, hipStream_t stream);
// The early part, on `side` while dgrad still runs: zeroes the replicas.  The caller has made `side` wait for its stream's earlier work.
int scatter_begin(const mnf_field_s *f, float *repl, bool deterministic, hipStream_t side);
// Everything else.  Leaves the walk's work on `side` (the caller joins it) and has `stream` wait for the bins.
int scatter_run(const ScatterCall &c);

}  // namespace mnf
