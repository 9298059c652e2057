// Radiance-field handle and the structs of the field's calls, shared by every unit that evaluates or trains the field.  field_api.hip owns the handle: it creates,
// fills (level table, fragment gather table) and destroys it and holds the forward's C entry points; field.hip holds the forward kernels and their launch per
// operand type; train.hip lazily attaches train_state; render.hip, trainstep.hip and occupancy.hip call launch_field.
#pragma once
#include <vector>

#include "common.h"

namespace mnf {

struct LevelMeta {
    float scale;
    uint32_t res;
    uint32_t size;    // entries in this level (tcnn params_in_level)
    uint32_t offset;  // first entry of this level in the table
    uint32_t hashed;  // 1: spatial hash, 0: dense
    // idx / size for any uint32 idx without a branch (dense levels wrap the index as tcnn does):
    // q = mulhi(div_magic, idx); q = (((idx - q) >> 1) + q) >> div_shift
    uint32_t div_magic, div_shift;
};

struct FieldShape {
    int W, NH, Wh, C;
    int blocks_total;  // 1 KiB fragment blocks of all nine weight matrices
};

}  // namespace mnf

struct mnf_field_s {
    mnf_field_config cfg;
    mnf::FieldShape shape;
    mnf::LevelMeta levels[16];
    int64_t table_entries;
    int64_t n_base_mlp, n_base, n_head, n_sem;  // fp32 parameter counts
    // device buffers owned by the handle
    void *d_table;       // fp16 [table_entries][4]
    void *d_frags;       // fp16 fragment-ordered MLP weights, blocks_total KiB
    int32_t *d_frag_src; // gather table: (buffer << 28) | index, or -1 for a structural zero
    int32_t *d_counter;  // work counter of the ray-major density pass (lazily allocated)
    bool params_loaded;
    std::vector<int32_t> frag_src_host;   // host copy of the gather table (train.hip inverts it: parameter -> fragment slot)
    void *train_state;        // lazily built by train.hip (transposed fragments, weight-gradient job table)
};
inline bool field_rows_supported(const mnf_field_s *f) { return f->cfg.neurons == 128 && !f->cfg.blend_fp16; }

namespace mnf {

// Per-round volumetric compositing fused into the field kernel's epilogue (mode 2): the renderer's tiles hold
// `nslots` rays x `stride` columns (a ray never straddles a 64-column tile), described by one header word per tile.
struct FusedRender {
    const int32_t *tile_hdr;      // [tiles]: columns per ray slot (= the budget of the tile's view this round) | view << 8
    uint8_t *alive;               // [rays]
    int32_t *alive_count;         // [views] survivors of this round
    const int32_t *n_samples;     // [views] this round's per-ray sample budget
    float *rgb, *acc, *depth, *sem, *rgb_var, *depth_var;   // running accumulators (the call's outputs)
    unsigned long long *totals;   // [2]: kept samples, evaluated samples
    int32_t rays_per_view, probabilistic;
    int32_t general_only;         // diagnostic (MNF_COMPOSITE_GENERAL=1): composite every tile with the general segmented-scan path
    int32_t tile_skip;            // 0: a tile without a kept sample stops behind the density (field.hip).  Diagnostic: 1 (MNF_NO_TILE_SKIP=1) no tile does,
                                  // 2 (MNF_TILE_SKIP_ALL=1) every tile does (wrong pictures: what a tile costs up to the density, on the same columns)
    uint32_t *diag_counts;        // diagnostic (MNF_ROUND_LOG, -DMNF_DIAG kernels only): [3] tiles without a kept sample | rays of the other tiles | those of them without a kept sample
    float alpha_thre, opc_thre;
};

// What the fused kernel reads / writes.  mode 0: explicit positions+directions; mode 1: packed samples
// with int64 ray indices; mode 2: renderer columns (int32 ray id, -1 = unused column); mode 3: mode 1 walked ray-major.
struct FieldIO {
    int mode;
    const float *positions, *directions;     // mode 0
    const float *rays_o, *rays_d;            // mode 1, 2
    const int64_t *ray_idx64;                // mode 1
    const int32_t *col_ray;                  // mode 2
    const float *t_starts, *t_ends;          // mode 1, 2
    int64_t n;                               // modes 0, 1
    const int32_t *n_dev;                    // mode 2: number of columns (device)
    int64_t n_cap;                           // mode 2: capacity of the column arrays (the device count is clamped to it)
    int32_t grid_limit;                      // mode 2: workgroups of this launch (0 = one per CU).  Render jobs that advance side by side share the chip:
                                             // each job's launch takes its share of the CUs, so the jobs' field kernels run BESIDE each other
    uint32_t *tickets;                       // mode 2, optional: eight zeroed counters 64 bytes apart.  The waves then take their tiles in the order they get to
                                             // them (one ticket per tile, range of XCD x first, then the next ranges) instead of a fixed stride
    const int64_t *n_dev64;                  // modes 0, 1, optional: the sample count lives on the device (`n` is then its upper
                                             // bound and sizes the launch): the train step never brings a count to the host
    // mode 3: packed samples walked ray by ray (ray_idx64 / t_starts / t_ends as mode 1) with early termination
    const int64_t *chunk_starts, *chunk_cnts;
    int32_t n_rays;
    int32_t *ray_counter;
    float sdt_stop;                          // stop a ray once its accumulated sigma * dt exceeds this
    // outputs: user layout (modes 0,1) ...
    float *rgb, *density, *sem;
    float *positions_out;                    // mode 1, optional: the sample positions [n,3] the kernel formed (the backward's scatter reads them)
    float *xn_out;                           // mode 1, optional: the aabb-normalised positions [n,3] (ngp.py:177-178) instead: the scatter's own input
    // ... or, in mode 2, composites straight into the renderer's per-ray accumulators
    FusedRender fr;
    // The train step's two passes over the hash table made one (neurons = 128, fp32 blend: field_rows_supported): the density pre-pass (mode 3) leaves every sample's
    // 64 encoded features behind as one 128-byte row, rows_out[sample] — exactly the 16-bit values its own MLP consumed — and the training forward (mode 1) reads
    // row rows_src[k] of rows_in for its sample k (one cache line) instead of gathering 128 table entries again.
    void *rows_out;
    const void *rows_in;
    const int64_t *rows_src;
    // modes 0, 1: `sem` class-major, sem[class * sem_stride + sample], instead of [sample][C] (0): a wave then writes 128-byte runs instead of 4-byte pieces at a
    // C * 4-byte lane stride (the train step's private logit buffer: 75 us of the 650 us training forward at 1.0 M samples were those stores)
    int64_t sem_stride;
};

// Training-time activation storage handed to the forward kernel (layout: field_dev.h, TrainLayout)
struct TrainBuf {
    void *act;        // [tiles][rows][64] 16-bit elements
    uint8_t *masks;   // [tiles][64 lanes][mask_bytes]: a record per lane (field_dev.h TrainLayout)
    int64_t Np;
    int32_t rows;
};

// What the backward leaves in the train workspace for the input gradients (inputgrad.hip): the un-scaled feature gradients, the normalised positions
// and the loss-scaled pre-activation gradients of the rgb head's first layer (rows row_dZr1 .. row_dZr1 + W/2 of `act`), plus the handle's map from
// the head's SH weights W1[j][k] (k < 16) to their slot in d_frags.
struct InputGradView {
    const void *act;          // [tiles][rows][64] 16-bit elements
    const float *dX;          // [16][Np][4]
    const float *xn;          // [n][3]
    int64_t Np;
    int32_t rows, row_dZr1;
    const int32_t *sh_slot;   // [W/2][16] device: index into d_frags
};

// The fused train render's ray gradients (inputgrad.hip train_render_ray_grad_kernel): what of the step's workspace the kernel reads beside the field's train
// workspace, and where the sums go.
struct RayGradIO {
    const float *xn;                              // [n][3] aabb-normalised positions of the kept samples
    const float *t_starts, *t_ends;               // [n]
    const int64_t *kept_starts, *kept_cnts;       // [n_rays]
    const int64_t *n_dev;                         // device: the surviving count the backward worked on
    const int32_t *skip;                          // device: the step's skip flag
    const float *rays_d;                          // [n_rays][3]; NULL without g_d
    int32_t n_rays;
    int64_t n;                                    // the sample arrays' bound (the field workspace was carved for it)
    float loss_scale;
    float *g_o, *g_d;                             // [n_rays][3] each, overwritten; either may be NULL
};

// The train step's output gradients in factored form: d_rgb[s] = w[s] * g_rgb[ray[s]], d_sem[s][c] = w[s] * g_sem[ray[s]][c] — what sem_rendering's backward
// (composite_train.hip) would write per sample, 128 bytes each at 29 classes, and the backward-data kernel would read back at a 116-byte lane stride.  Given the
// factors the kernel forms the products itself (same fp32 multiplications): 12 bytes per sample plus per-ray vectors that stay in cache.
struct FactoredGrad { const float *w; const int64_t *ray; const float *g_rgb, *g_sem; };

// One call of the field's backward (train.hip)
struct BackwardCall {
    const float *positions;                      // [n][3]: world positions, or aabb-normalised ones (positions_normalized)
    int64_t n; const int64_t *n_dev;             // samples, and optionally their count on the device (n = its upper bound)
    const float *d_rgb, *d_density, *d_sem;      // output gradients [n][3], [n], [n][C]; d_rgb / d_sem are not read when `factored` is given
    const float *rgb, *density;                  // forward outputs [n][3], [n]
    void *workspace; int64_t workspace_bytes;    // the train workspace the forward filled (mnf_field_train_workspace_bytes)
    float loss_scale;
    float *g_base, *g_head, *g_sem;              // fp32 parameter gradients, added to; all three NULL: none (frozen parameters), the call stops behind dgrad
    bool zero_grads, positions_normalized;       // zero the three vectors first; see `positions`
    bool deterministic;                          // fixed-point table gradient, ordered weight-gradient partial sums
    FactoredGrad factored;                       // all NULL: absent
    hipStream_t stream;
};

// dispatchers on the handle's operand type, defined once: launch_field in field_api.hip, the others in the fp16 translation unit of train.hip / inputgrad.hip
void free_train_state(mnf_field_t f);
int launch_field(mnf_field_t f, const FieldIO &io, bool density_only, hipStream_t stream, const TrainBuf *train = nullptr);
// training forward / backward
int forward_train(mnf_field_t f, const FieldIO &io, void *workspace, int64_t workspace_bytes, hipStream_t stream, bool deterministic = false);
int backward(mnf_field_t f, const BackwardCall &c);
int train_render_ray_grad(mnf_field_t f, void *field_ws, const RayGradIO &io, hipStream_t stream);

#define MNF_DECLARE_DT_IMPL(ns)                                                                                                      \
    namespace ns {                                                                                                                   \
    int launch_field_impl(mnf_field_t f, const FieldIO &io, bool density_only, hipStream_t stream, const TrainBuf *train);           \
    int set_params_impl(mnf_field_t f, const float *mlp_base, const float *mlp_head, const float *mlp_sem, bool table_current,       \
                        hipStream_t stream);                                                                                         \
    void free_train_state_impl(mnf_field_t f);                                                                                       \
    int64_t train_workspace_bytes_impl(mnf_field_t f, int64_t n);                                                                    \
    int forward_train_impl(mnf_field_t f, const FieldIO &io, void *workspace, int64_t workspace_bytes, hipStream_t stream,          \
                           bool deterministic);                                                                                      \
    int backward_impl(mnf_field_t f, const BackwardCall &c);                                                                         \
    int input_grad_view_impl(mnf_field_t f, void *workspace, int64_t n, InputGradView &view);                                        \
    int field_input_grad_impl(mnf_field_t f, const InputGradView &view, const float *directions, int64_t n, float loss_scale,       \
                              float *d_positions, float *d_directions, hipStream_t stream);                                          \
    int train_render_ray_grad_impl(mnf_field_t f, void *field_ws, const RayGradIO &io, hipStream_t stream);                          \
    }
MNF_DECLARE_DT_IMPL(f16)
MNF_DECLARE_DT_IMPL(bf16)

}  // namespace mnf
