/*
 * mi355nerf.h — C ABI of libmi355nerf.so, the MI355X (gfx950) implementation of the
 * reference's perception hot path.
 *
 * The reference has no FFI of its own: its native layer is (1) the pybind11 module
 * `nerfacc_cuda` (perception/nerfacc/nerfacc/cuda/csrc/nerfacc.cpp:100-128) and (2) the
 * un-vendored `tinycudann` torch extension (perception/models/radiance_fields/ngp.py:108-169).
 * Each entry point below names the reference interface it replaces.  INTEGRATION.md shows the
 * ctypes binding a maintainer adds on the reference side.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the parameter name ends in `_host`;
 *     buffers are caller-owned, the library allocates nothing per call except inside handles;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); every call only
 *     enqueues work unless documented otherwise;
 *   - return value 0 = ok, negative = error; text via mnf_last_error() (thread-local);
 *   - handles are thread-compatible, not thread-safe;
 *   - there is NO CPU fallback: without a HIP device every compute entry point fails.
 */
#ifndef MI355NERF_H
#define MI355NERF_H

#include <stdint.h>
#include <string.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MNF_OK 0
#define MNF_ERR_INVALID (-1)
#define MNF_ERR_HIP (-2)
#define MNF_ERR_UNSUPPORTED (-3)
#define MNF_ERR_WORKSPACE (-4)

typedef void *mnf_stream_t;
typedef struct mnf_field_s *mnf_field_t;

const char *mnf_last_error(void);
int mnf_version(void);
/* number of visible HIP devices (0 when there is none; never initialises a context) */
int mnf_device_count(void);

/* ---------------------------------------------------------------- nerfacc_cuda replacements */

/* nerfacc.cpp:110 `ray_aabb_intersect` (grid.cu:477-519, kernel :284-313).
 * t_mins,t_maxs [n_rays,n_aabbs] f32; hits [n_rays,n_aabbs] u8 (torch.bool layout). */
int mnf_ray_aabb_intersect(const float *rays_o, const float *rays_d, int32_t n_rays,
                           const float *aabbs, int32_t n_aabbs,
                           float near_plane, float far_plane, float miss_value,
                           float *t_mins, float *t_maxs, uint8_t *hits, mnf_stream_t stream);

/* One launch of the reference's `traverse_grids_kernel` (grid.cu:68-282); the host-side
 * count / cumsum / fill protocol of grid.cu:320-474 is driven by the caller exactly as the
 * reference's C++ does (first_pass=1 writes chunk_cnts only; first_pass=0 fills at
 * chunk_starts and rewrites chunk_cnts with the actual counts).  Pointers of a disabled output
 * are NULL (iv_chunk_cnts==NULL disables intervals, sm_chunk_cnts==NULL disables samples).
 * binaries [n_grids,X,Y,Z] u8; t_indices/ray_indices/chunk_* are int64 as in the reference. */
int mnf_traverse_grids(const float *rays_o, const float *rays_d, const uint8_t *rays_mask, int32_t n_rays,
                       const uint8_t *binaries, const float *aabbs, int32_t n_grids,
                       int32_t res_x, int32_t res_y, int32_t res_z,
                       const uint8_t *hits, const float *t_sorted, const int64_t *t_indices,
                       const float *near_planes, const float *far_planes,
                       float step_size, float cone_angle, int32_t traverse_steps_limit, int32_t first_pass,
                       float *iv_vals, int64_t *iv_ray_indices, uint8_t *iv_is_left, uint8_t *iv_is_right,
                       const int64_t *iv_chunk_starts, int64_t *iv_chunk_cnts,
                       float *sm_vals, int64_t *sm_ray_indices, uint8_t *sm_is_valid,
                       const int64_t *sm_chunk_starts, int64_t *sm_chunk_cnts,
                       float *terminate_planes, mnf_stream_t stream);

/* Single-pass form of the sampling traversal for one grid level (what `OccGridEstimator.sampling`,
 * occ_grid.py:80-238, needs from `traverse_grids`): every ray is marched ONCE; its samples (t_start, t_end) go to row r of
 * the caller's scratch [n_rays][cap] and counts[r] receives the ray's full sample count (rows are truncated at cap:
 * if any count exceeds cap the caller falls back to mnf_traverse_grids).  aabb_host: 6 host floats.  bitgrid: optional
 * bit-packed form of `binaries` (mnf_pack_bitgrid / mnf_occ_binarize; NULL = packed from the bytes by every workgroup).
 * The t values are those of mnf_traverse_grids, bit for bit. */
int mnf_sample_rays(const float *rays_o, const float *rays_d, int32_t n_rays, const uint8_t *binaries, int32_t res_x,
                    int32_t res_y, int32_t res_z, const float *aabb_host, const float *near_planes, const float *far_planes,
                    float step_size, float cone_angle, int32_t cap, float *scratch_ts, float *scratch_te, int64_t *counts,
                    const uint32_t *bitgrid, mnf_stream_t stream);
/* The same over n_levels (1..4) occupancy levels (occ_grid.py:37-55; grid.cu:125-151 takes a ray's segments level by level):
 * binaries [n_levels,X,Y,Z], aabb_host n_levels x 6 floats (estimator.aabbs), bitgrid [n_levels][ceil(cells / 32)] words. */
int mnf_sample_rays_levels(const float *rays_o, const float *rays_d, int32_t n_rays, const uint8_t *binaries, int32_t n_levels,
                           int32_t res_x, int32_t res_y, int32_t res_z, const float *aabb_host, const float *near_planes,
                           const float *far_planes, float step_size, float cone_angle, int32_t cap, float *scratch_ts, float *scratch_te,
                           int64_t *counts, const uint32_t *bitgrid, mnf_stream_t stream);

/* Pack the scratch rows: samples of ray r go to [chunk_starts[r], chunk_starts[r] + counts[r]) of t_starts / t_ends /
 * ray_indices (chunk_starts = exclusive prefix of counts, `RaySegmentsSpec::memalloc_data_from_chunk`, data_spec.hpp:86-96). */
int mnf_compact_samples(const float *scratch_ts, const float *scratch_te, int32_t cap, const int64_t *chunk_starts,
                        const int64_t *counts, int32_t n_rays, float *t_starts, float *t_ends, int64_t *ray_indices,
                        mnf_stream_t stream);

/* nerfacc.cpp:104 `exclusive_sum` (scan.cu:68-125); backward=1 is the reverse-direction scan
 * used by the autograd rule (scan.py:226-228). */
int mnf_exclusive_sum(const int64_t *chunk_starts, const int64_t *chunk_cnts, int32_t n_rays,
                      const float *inputs, float *outputs, int64_t n_edges, int32_t backward,
                      mnf_stream_t stream);

/* Fused render_weight_from_density (volrend.py:315-365) on packed samples:
 * weights = T*alpha, trans, alphas with an optional per-sample prefix transmittance (may be NULL). */
int mnf_render_weight_from_density(const int64_t *chunk_starts, const int64_t *chunk_cnts, int32_t n_rays,
                                   const float *t_starts, const float *t_ends, const float *sigmas,
                                   const float *prefix_trans, int64_t n_samples,
                                   float *weights, float *trans, float *alphas, mnf_stream_t stream);

/* The tail of `OccGridEstimator.sampling` (occ_grid.py:209-236): render_visibility_from_density (volrend.py:424-483: T >= early_stop_eps and
 * alpha >= alpha_thre) and the three boolean-mask selections after it, on packed samples, in two passes around one prefix sum:
 *   count pass (o_t_starts NULL): kept_cnts[r] = survivors of ray r;
 *   write pass: kept_starts = exclusive scan of kept_cnts; survivors go to o_*[kept_starts[r] ...], grouped by ray in marching order.
 * alpha_thre_dev: ONE float on the device — min(alpha_thre, occs.mean()) of occ_grid.py:211 without the host round trip. */
int mnf_visible_samples(const int64_t *chunk_starts, const int64_t *chunk_cnts, int32_t n_rays, const float *t_starts, const float *t_ends,
                        const float *sigmas, float early_stop_eps, const float *alpha_thre_dev, int64_t *kept_cnts, const int64_t *kept_starts,
                        float *o_t_starts, float *o_t_ends, int64_t *o_ray_indices, mnf_stream_t stream);

/* Run boundaries of ray indices that are grouped by ray (the marcher's output order): first[r] = index of the
 * first sample of ray r, last[r] = one past its last sample; both must be zero-filled by the caller, rays without
 * samples stay (0, 0).  cnts = last - first is `pack_info`'s second column (nerfacc/pack.py:10-38). */
int mnf_run_bounds(const int64_t *ray_indices, int64_t n_samples, int64_t *first, int64_t *last, mnf_stream_t stream);

/* Train-mode semantic volume rendering on packed samples (perception/models/utils.py:362-461 `sem_rendering`):
 * render_weight_from_density (volrend.py:213-267) + the four accumulate_along_rays (volrend.py:27-66) + background
 * blend + depth normalisation in one launch.  Outputs: rgb [R,3], acc [R], depth [R], sem [R,C]; per-sample weights and
 * trans [N] are saved for backward, alphas is optional.  bkgd (3 floats, device) may be NULL.  n_classes <= 64. */
int mnf_composite_train_forward(const int64_t *chunk_starts, const int64_t *chunk_cnts, int32_t n_rays,
                                const float *t_starts, const float *t_ends, const float *sigmas, const float *rgbs,
                                const float *sems, int32_t n_classes, int64_t n_samples, const float *bkgd,
                                float *out_rgb, float *out_acc, float *out_depth, float *out_sem, float *weights,
                                float *trans, float *alphas, mnf_stream_t stream);

/* Its adjoint (what torch autograd derives for the reference's op chain): gradients of the four per-ray outputs
 * (any of g_* may be NULL = zero) -> d_sigmas [N], d_rgbs [N,3], d_sems [N,C].  d_rgbs and d_sems may BOTH be NULL: they are
 * weights[s] * g_rgb[ray] and weights[s] * g_sem[ray], which a caller that has the weights can form itself (mnf_train_step's
 * backward-data kernel does: 128 bytes per sample less to write and to read back). */
int mnf_composite_train_backward(const int64_t *chunk_starts, const int64_t *chunk_cnts, int32_t n_rays,
                                 const float *t_starts, const float *t_ends, const float *sigmas, const float *rgbs,
                                 const float *sems, int32_t n_classes, int64_t n_samples, const float *bkgd,
                                 const float *weights, const float *trans, const float *out_acc,
                                 const float *out_depth, const float *g_rgb, const float *g_acc, const float *g_depth,
                                 const float *g_sem, float *d_sigmas, float *d_rgbs, float *d_sems, mnf_stream_t stream);

/* One `torch.optim.Adam` step (weight_decay 0, amsgrad off: scripts/pipeline.py:173-178, :531) on a flat fp32
 * parameter vector in a single pass; `step` counts from 1.  State buffers are the optimizer's exp_avg / exp_avg_sq. */
int mnf_adam_step(float *params, const float *grads, float *exp_avg, float *exp_avg_sq, int64_t n, float lr, float beta1,
                  float beta2, float eps, int32_t step, mnf_stream_t stream);

/* The same step for a training loop that never synchronises with the host (scripts/pipeline.py:520-532 decided on the device):
 * step_dev (device float, torch's `state["step"]`) is advanced and the update applied only when *skip_dev == 0 (skip_dev: device
 * int32 or NULL; raised by mnf_count_nan for non-finite gradients and by mnf_train_step for a step without samples or beyond its
 * bounds).  hyper_dev: 4 device floats of scratch.  half_out / half_from: optional fp16 mirror — parameters half_from.. are also
 * written, rounded to fp16, to half_out[0..] (the field handle's hash table, mnf_field_table_mirror: no per-step conversion pass). */
int mnf_adam_step_guarded(float *params, const float *grads, float *exp_avg, float *exp_avg_sq, int64_t n, float lr, float beta1,
                          float beta2, float eps, float *step_dev, const int32_t *skip_dev, float *hyper_dev, void *half_out,
                          int64_t half_from, mnf_stream_t stream);

/* scripts/pipeline.py:520-532 for one model as ONE call: non-finite-gradient guard over the three parameter vectors of a field (added to
 * *skip_dev when count_nonfinite != 0), the three mnf_adam_step_guarded updates (mlp_base / mlp_head / mlp_sem, in that order: host arrays
 * of 3 device pointers each; the hash table's fp16 mirror in the handle is written by the update), then the handle's MLP weight fragments
 * are re-derived: after the call the handle is current for the new parameters.  hyper_dev: 12 device floats of scratch. */
int mnf_field_optimizer_step(mnf_field_t f, float *const *params_host, const float *const *grads_host, float *const *exp_avg_host,
                             float *const *exp_avg_sq_host, float *const *step_dev_host, float lr, float beta1, float beta2, float eps,
                             int32_t *skip_dev, int32_t count_nonfinite, float *hyper_dev, mnf_stream_t stream);
/* The same call with the step's report to the host: counts_dev (mnf_train_step's 4 device counters, or NULL) and the final value of *skip_dev are written by the
 * step-count kernel straight into report_host — 5 x int64 of PINNED host memory (device-accessible) — behind the non-finite count: an asynchronous training loop
 * learns sample counts and skipped steps without a device-to-host copy on the stream (each such copy cost the stream ~25 us).  Readable once an event recorded
 * behind the call has completed. */
int mnf_field_optimizer_step_report(mnf_field_t f, float *const *params_host, const float *const *grads_host, float *const *exp_avg_host,
                                    float *const *exp_avg_sq_host, float *const *step_dev_host, float lr, float beta1, float beta2, float eps,
                                    int32_t *skip_dev, int32_t count_nonfinite, float *hyper_dev, const int64_t *counts_dev,
                                    int64_t *report_host, mnf_stream_t stream);

/* Adds the number of NaN / Inf entries of `values` to *count (device int32): the gradient guard of pipeline.py:520-529. */
int mnf_count_nan(const float *values, int64_t n, int32_t *count, mnf_stream_t stream);

/* `pack_info` (nerfacc/pack.py:10-38) for ray indices in any order: packed_info [n_rays,2] = (chunk start, chunk count).
 * workspace: 2*n_rays*8 + mnf_scan_workspace_bytes(n_rays) bytes. */
int64_t mnf_scan_workspace_bytes(int64_t n);
int mnf_pack_info(const int64_t *ray_indices, int64_t n_samples, int64_t n_rays, int64_t *packed_info, void *workspace,
                  int64_t workspace_bytes, mnf_stream_t stream);
/* Exclusive prefix sum of int64 counts (chunk starts of `RaySegmentsSpec::memalloc_data_from_chunk`,
 * include/data_spec.hpp:86-96); total_out (device, optional) receives the grand total. */
int mnf_exclusive_scan_i64(const int64_t *in, int64_t n, int64_t *out, int64_t *total_out, void *workspace, int64_t workspace_bytes,
                           mnf_stream_t stream);

/* `accumulate_along_rays` / `accumulate_along_rays_` with ray_indices (nerfacc/volrend.py:486-576): outputs [n_rays,dim]
 * (caller-initialised) += weights[k] * values[k,:] at row ray_indices[k]; values NULL = weights alone (dim 1).
 * The backward gives what autograd derives for the reference's index_add_: grad_weights [n] and grad_values [n,dim]
 * (either may be NULL) from grad_outputs [n_rays,dim]. */
int mnf_accumulate_along_rays(const float *weights, const float *values, const int64_t *ray_indices, int64_t n_samples, int32_t dim,
                              float *outputs, mnf_stream_t stream);
int mnf_accumulate_along_rays_backward(const float *weights, const float *values, const int64_t *ray_indices, int64_t n_samples,
                                       int32_t dim, const float *grad_outputs, float *grad_weights, float *grad_values,
                                       mnf_stream_t stream);

/* ---------------------------------------------------------------- occupancy-grid refresh
 * `OccGridEstimator._update` (nerfacc/estimators/occ_grid.py:345-437) without host round trips.  A refresh of one level is
 *   mnf_occ_sample_cells -> (density of the points: occ_eval_fn) -> mnf_occ_apply, then mnf_occ_binarize over all levels;
 * mnf_update_occupancy does the whole chain for one level with the field's own density kernel as occ_eval_fn
 * (scripts/pipeline.py:376-378: query_density(x) * render_step_size).
 * The sample list has a fixed capacity (mnf_occ_list_capacity: every cell during warm-up, 2 * (cells / 4) afterwards);
 * unused slots hold cell index -1 and a point inside the box (the box centre); a capacity of 0 — fewer than four cells past
 * the warm-up — is valid: nothing is written and cell_idx / points may be NULL.  Draws: Philox4x32-10, counter (element, 0, kind, step),
 * key = seed, kind 0 uniform / 1 occupied / 2 warm-up; word 0 -> cell, words 1..3 -> in-cell offsets (24-bit).  Tests
 * pass the reference's recorded draws instead (indices_in, jitter_in [n_in,3]).  Duplicate cells: the last list element
 * wins.  workspace: mnf_occ_workspace_bytes(cells, fused), the same buffer for sample and apply of one refresh. */
int64_t mnf_occ_workspace_bytes(int64_t cells_per_level, int32_t fused);
int64_t mnf_occ_list_capacity(int64_t cells_per_level, int32_t step, int32_t warmup_steps);
/* binaries [levels, cells] u8 -> bitgrid [levels, ceil(cells/32)] (bit c & 31 of word c >> 5) */
int mnf_pack_bitgrid(const uint8_t *binaries, int64_t cells_per_level, int32_t levels, uint32_t *bitgrid, mnf_stream_t stream);
int mnf_occ_sample_cells(const float *occs, const uint32_t *bitgrid, int32_t res_x, int32_t res_y, int32_t res_z,
                         const float *aabb_host, int32_t step, int32_t warmup_steps, uint64_t seed,
                         const int64_t *indices_in, const float *jitter_in, int64_t n_in,
                         int64_t *cell_idx, float *points, int64_t capacity, void *workspace, int64_t workspace_bytes,
                         mnf_stream_t stream);
/* occs[cell] = max(occs[cell] * ema_decay, values[e] * value_scale), NaN candidates leave the cell unchanged (occ_grid.py:403-434) */
int mnf_occ_apply(float *occs, const int64_t *cell_idx, const float *values, float value_scale, int64_t n, int64_t cells_per_level,
                  float ema_decay, void *workspace, int64_t workspace_bytes, mnf_stream_t stream);
/* thre = min(mean(occs[occs >= 0]), occ_thre); binaries = occs > thre as bytes and as bits (occ_grid.py:436-437);
 * threshold_out (device float, optional) receives thre */
int mnf_occ_binarize(const float *occs, int64_t cells_per_level, int32_t levels, float occ_thre, uint8_t *binaries,
                     uint32_t *bitgrid, float *threshold_out, void *workspace, int64_t workspace_bytes, mnf_stream_t stream);
int mnf_update_occupancy(mnf_field_t f, float *occs, uint8_t *binaries, uint32_t *bitgrid, int32_t res_x, int32_t res_y,
                         int32_t res_z, const float *aabb_host, int32_t step, int32_t warmup_steps, float occ_thre,
                         float ema_decay, float density_scale, uint64_t seed, void *workspace, int64_t workspace_bytes,
                         mnf_stream_t stream);

/* ---------------------------------------------------------------- ray generation */

/* Dataset.generate_image_rays (perception/data_proc/habitat_to_data.py:274-301) for n_views poses,
 * restricted to the flat pixel indices pix_idx[n_pix] (int64; the np.round(np.linspace(...))
 * sub-sampler of :462-467 is evaluated by the caller on the host in float64, as the reference does;
 * NULL = all width*height pixels).  c2w [n_views,3,4] row-major f32.
 * origins, viewdirs [n_views, n_pix, 3] f32. */
int mnf_generate_rays(const float *c2w, int32_t n_views, int32_t width, int32_t height, float focal,
                      const int64_t *pix_idx, int64_t n_pix, float *origins, float *viewdirs,
                      mnf_stream_t stream);

/* Dataset.fetch_data's pixel gather (habitat_to_data.py:229-232) for ONE image: rgb [n,3] f32 = images[id, pix] / 255.0,
 * dep [n] f32, sem [n] i64 at the flat pixel indices pix_idx (y * W + x).  images [N,H,W,3] u8; depths [N,H,W] f32
 * (reference storage) or f16 (packed layout, depth_is_f16 = 1); semantics [N,H,W] i64 or u8 (sem_is_u8 = 1); image_id:
 * ONE int64 on the device (the reference draws it with torch.randint on the device). */
int mnf_gather_pixels(const uint8_t *images, const void *depths, int32_t depth_is_f16, const void *semantics, int32_t sem_is_u8,
                      int64_t pixels_per_image, const int64_t *image_id, const int64_t *pix_idx, int64_t n_pix, float *rgb,
                      float *dep, int64_t *sem, mnf_stream_t stream);

/* ---------------------------------------------------------------- radiance field (tinycudann replacement) */

/* Structs that the library takes BY POINTER (mnf_field_config, mnf_vanilla_config, mnf_train_opts, mnf_render_opts, and every element of a mnf_render_job
 * array) start with `struct_size`: set it to sizeof(the struct) (MNF_INIT below zero-fills and sets it).
 * The library refuses any other value (MNF_ERR_INVALID), so a caller compiled against an older header — whose struct is shorter than what this
 * library reads — is stopped at the boundary instead of having the tail of its struct read from whatever follows it.  Every field added after a
 * struct's first release reads 0 / NULL as "the previous behaviour". */
#define MNF_INIT(var) do { memset(&(var), 0, sizeof(var)); (var).struct_size = (uint32_t)sizeof(var); } while (0)

typedef struct {
    uint32_t struct_size;          /* sizeof(mnf_field_config) */
    float aabb[6];                 /* ngp.py:91 */
    int32_t neurons;               /* ngp.py:77  (64 or 128) */
    int32_t layers;                /* ngp.py:78  == tcnn n_hidden_layers of the base MLP (>=1) */
    int32_t num_semantic_classes;  /* ngp.py:87  (1..32) */
    int32_t n_levels;              /* ngp.py:84  (must be 16) */
    int32_t n_features;            /* ngp.py:127 (must be 4) */
    int32_t log2_hashmap_size;     /* ngp.py:85 */
    int32_t base_resolution;       /* ngp.py:81 */
    int32_t max_resolution;        /* ngp.py:82 */
    int32_t output_fp16;           /* 0 (default): network outputs stay fp32.  1: every output of the three networks is rounded
                                      to fp16 before it is used, as tiny-cuda-nn hands them over (ngp.py:181-200, :210-220 cast
                                      tcnn's fp16 outputs back with `.to(x)`) — the tcnn-faithful mode of DESIGN.md §2 */
    int32_t mfma_bf16;             /* 0 (default): fp16 matrix-core operands (weights, MLP inputs, activations and their gradients), the
                                      reference's tiny-cuda-nn arithmetic.  1: bf16 operands (BASELINE config 5); the hash table stays
                                      fp16, accumulation fp32 */
    int32_t blend_fp16;            /* 0 (default): the 8-corner blend of a hash level runs in fp32 (fp32 weight x widened fp16 entry, fp32 sum, ONE rounding
                                      to the 16-bit MLP input).  1: tiny-cuda-nn's own arithmetic as published (grid encoding instantiated with T = __half
                                      behind a half-precision network): the corner weight is rounded to fp16 and the sum runs as fp16 fused multiply-adds,
                                      `result = fma((T)weight, entry, result)`, corners in index order (x fastest) — packed v_pk_fma_f16 on the two
                                      feature pairs.  Changes features by ~1e-3 relative; which one the reference's un-pinned tinycudann build computes
                                      cannot be verified in this container. */
} mnf_field_config;

/* tcnn.NetworkWithInputEncoding / tcnn.Network / tcnn.Encoding construction, ngp.py:108-169 */
int mnf_field_create(const mnf_field_config *cfg, mnf_field_t *out);
int mnf_field_destroy(mnf_field_t f);
/* number of fp32 parameters of module `which` (0 = mlp_base incl. hash table, 1 = mlp_head, 2 = mlp_sem),
 * i.e. the length of the reference state_dict entry `<module>.params` */
int64_t mnf_field_param_count(mnf_field_t f, int32_t which);
/* per-level metadata for tests: out arrays of n_levels entries (HOST pointers) */
int mnf_field_grid_meta_host(mnf_field_t f, float *scale_host, int32_t *res_host, int32_t *size_host,
                             int64_t *offset_host, int32_t *hashed_host);
/* Load fp32 master parameters (device pointers, reference state_dict layout) and build the fp16
 * hash table and MFMA-fragment-ordered fp16 weights held by the handle. */
int mnf_field_set_params(mnf_field_t f, const float *mlp_base, const float *mlp_head, const float *mlp_sem,
                         mnf_stream_t stream);
/* The handle's fp16 hash table as an optimizer mirror: device pointer to [entries][4] fp16; *first_param_host receives the index of
 * the first table entry inside `mlp_base.params` (the base-MLP weights precede it, ngp.py:123-141).  An optimizer that writes the
 * rounded new table values there (mnf_adam_step_guarded) calls mnf_field_refresh_weights afterwards instead of
 * mnf_field_set_params: only the few-KB MLP fragments are rebuilt. */
void *mnf_field_table_mirror(mnf_field_t f, int64_t *first_param_host);
int mnf_field_refresh_weights(mnf_field_t f, const float *mlp_base, const float *mlp_head, const float *mlp_sem, mnf_stream_t stream);

/* NGPRadianceField.forward (ngp.py:222-238): positions,directions [n,3] f32 ->
 * rgb [n,3], density [n,1], sem [n,C] f32 (any output may be NULL). */
int mnf_field_forward(mnf_field_t f, const float *positions, const float *directions, int64_t n,
                      float *rgb, float *density, float *sem, mnf_stream_t stream);
/* NGPRadianceField.query_density (ngp.py:171-200): density [n,1] */
int mnf_field_density(mnf_field_t f, const float *positions, int64_t n, float *density, mnf_stream_t stream);
/* the closures sigma_fn / rgb_sigma_sem_fn of utils.py:89-137 fused with the field:
 * positions = o[ray] + d[ray]*(t_start+t_end)/2, directions = d[ray]; ray_indices int64 */
int mnf_field_forward_samples(mnf_field_t f, const float *rays_o, const float *rays_d,
                              const int64_t *ray_indices, const float *t_starts, const float *t_ends, int64_t n,
                              float *rgb, float *density, float *sem, mnf_stream_t stream);

/* The density pre-pass of `OccGridEstimator.sampling` (occ_grid.py:196-233: sigma_fn on every marched sample, then
 * render_visibility_from_density) with the work behind opaque surfaces left out: samples are packed by ray
 * (chunk_starts / chunk_cnts [n_rays] int64, as traverse_grids returns them); a ray is evaluated front to back and the
 * rest of it is skipped once its transmittance has fallen below early_stop_eps / 2 — those samples fail the visibility
 * test whatever their density, so `density` (zero there) yields the same mask.  early_stop_eps <= 0 evaluates everything. */
int mnf_field_density_rays(mnf_field_t f, const float *rays_o, const float *rays_d, const int64_t *ray_indices,
                           const float *t_starts, const float *t_ends, const int64_t *chunk_starts, const int64_t *chunk_cnts,
                           int32_t n_rays, int64_t n_samples, float early_stop_eps, float *density, mnf_stream_t stream);

/* ---------------------------------------------------------------- frequency-encoded MLP field (BASELINE config 1)
 * perception/models/radiance_fields/mlp.py: `VanillaNeRFRadianceField` (:206-245) = `SinusoidalEncoder` (:168-203, 10 degrees
 * on positions, 4 on directions, identity included) + `NerfMLP` (:113-165) of biased Linear + ReLU layers (:14-101), in
 * exact fp32 on the matrix cores.  Parameters cross the boundary as ONE flat fp32 vector in the order of the reference's
 * `named_parameters()`: per Linear its weight [out][in] then its bias — base hidden layers, sigma layer, bottleneck layer,
 * rgb hidden layers, rgb output layer (mnf_vanilla_param_layout_host lists the tensors). */
typedef struct mnf_vanilla_s *mnf_vanilla_t;
typedef struct {
    uint32_t struct_size;         /* sizeof(mnf_vanilla_config), see MNF_INIT */
    int32_t net_depth;            /* mlp.py:209 */
    int32_t net_width;            /* mlp.py:210 (multiple of 32) */
    int32_t skip_layer;           /* mlp.py:211; <= 0 = None */
    int32_t net_depth_condition;  /* mlp.py:212 (>= 1) */
    int32_t net_width_condition;  /* mlp.py:213 (multiple of 32) */
} mnf_vanilla_config;
int mnf_vanilla_create(const mnf_vanilla_config *cfg, mnf_vanilla_t *out);
int mnf_vanilla_destroy(mnf_vanilla_t v);
int64_t mnf_vanilla_param_count(mnf_vanilla_t v);
/* offsets / rows / cols of the parameter tensors inside the flat vector, in named_parameters() order (host arrays of
 * max_tensors entries; *n_tensors_host receives the count) */
int mnf_vanilla_param_layout_host(mnf_vanilla_t v, int32_t max_tensors, int32_t *n_tensors_host, int64_t *offsets_host,
                                  int32_t *rows_host, int32_t *cols_host);
int mnf_vanilla_set_params(mnf_vanilla_t v, const float *flat_params, mnf_stream_t stream);
int64_t mnf_vanilla_train_workspace_bytes(mnf_vanilla_t v, int64_t n);
/* VanillaNeRFRadianceField.forward (mlp.py:238-243): positions [n,3]; directions [ceil(n / samples_per_direction),3] (the
 * reference broadcasts a per-ray condition over the ray's samples, mlp.py:154-160; 1 = one direction per sample);
 * rgb [n,3] = sigmoid, sigma [n] = relu.  workspace non-NULL (mnf_vanilla_train_workspace_bytes) keeps the activations for
 * mnf_vanilla_backward. */
int mnf_vanilla_forward(mnf_vanilla_t v, const float *positions, const float *directions, int64_t n,
                        int32_t samples_per_direction, float *rgb, float *sigma, void *workspace, int64_t workspace_bytes,
                        mnf_stream_t stream);
/* VanillaNeRFRadianceField.query_density (mlp.py:233-236) */
int mnf_vanilla_density(mnf_vanilla_t v, const float *positions, int64_t n, float *sigma, mnf_stream_t stream);
/* gradients of all parameters (flat, overwritten) from dL/d(rgb) [n,3] and dL/d(sigma) [n]; rgb / sigma are the forward
 * outputs, workspace the one the forward filled */
int mnf_vanilla_backward(mnf_vanilla_t v, const float *d_rgb, const float *d_sigma, const float *rgb, const float *sigma,
                         int64_t n, void *workspace, int64_t workspace_bytes, float *grad_flat, mnf_stream_t stream);

/* ---------------------------------------------------------------- training: differentiable field
 * What `loss.backward()` reaches inside tiny-cuda-nn in the reference (scripts/pipeline.py:518): the forward
 * that keeps activations and the backward to the flat parameter vectors.  Compositing, the loss and the optimizer
 * stay with the caller exactly as in the reference (perception/models/utils.py:362-461, pipeline.py:506-535). */

/* The backward behind the train forward is tiny-cuda-nn's own decomposition (ngp.py:123-169 / pipeline.py:518): a fused backward-data kernel (dgrad) and
 * weight-gradient GEMMs (wgrad) over the 2.4 KB per sample of 16-bit activations the train forward saves.  (A single-kernel form without the dump was built in
 * round 4 and measured slower: tools/experiments/fused_backward.patch, DESIGN.md "negative results".) */
/* bytes of workspace the train forward/backward pair needs for n samples (activations, masks, feature gradients) */
int64_t mnf_field_train_workspace_bytes(mnf_field_t f, int64_t n);
/* NGPRadianceField.forward with activations saved into `workspace` for the following backward */
int mnf_field_forward_train(mnf_field_t f, const float *positions, const float *directions, int64_t n,
                            float *rgb, float *density, float *sem, void *workspace, int64_t workspace_bytes,
                            mnf_stream_t stream);
/* Backward of the forward above: d_rgb [n,3], d_density [n], d_sem [n,C] are dL/d(outputs); rgb/density are the
 * forward outputs; `workspace` is the one the forward filled.  g_base / g_head / g_sem receive dL/d(params) in the
 * state_dict layout (fp32, overwritten).  Activation gradients are carried in fp16 scaled by loss_scale (tcnn's
 * default is 128); the returned gradients are un-scaled.  The parameters are the ones last passed to
 * mnf_field_set_params (the handle holds its own fp16 copies; the caller's vectors need not be alive). */
int mnf_field_backward(mnf_field_t f, const float *positions, int64_t n,
                       const float *d_rgb, const float *d_density, const float *d_sem,
                       const float *rgb, const float *density,
                       void *workspace, int64_t workspace_bytes, float loss_scale,
                       float *g_base, float *g_head, float *g_sem, mnf_stream_t stream);

/* mnf_field_forward_train for packed samples given as (ray, t_start, t_end): positions are formed in the kernel as the closure of
 * utils.py:122-137 does (origins + dirs * (t_starts + t_ends) / 2) and also written to positions_out [n,3], which
 * mnf_field_backward takes as `positions`. */
int mnf_field_forward_train_samples(mnf_field_t f, const float *rays_o, const float *rays_d, const int64_t *ray_indices,
                                    const float *t_starts, const float *t_ends, int64_t n, float *rgb, float *density,
                                    float *sem, float *positions_out, void *workspace, int64_t workspace_bytes,
                                    mnf_stream_t stream);

/* ---------------------------------------------------------------- training: gradients with respect to the field's inputs
 * tiny-cuda-nn returns dL/d(input) of its encodings and networks behind `loss.backward()` (scripts/pipeline.py:518; the modules of
 * perception/models/radiance_fields/ngp.py:123-169): the gradient a pose refiner needs with the parameters frozen.
 *
 * mnf_field_backward_inputs replaces that input gradient for NGPRadianceField.forward: d_positions [n,3] and / or d_directions [n,3]
 * (either may be NULL, fp32, overwritten) from what mnf_field_backward left in `workspace`.  Call it after mnf_field_backward with the
 * same f, n, workspace and loss_scale; nothing in between may write the workspace or reload weights (the head weights are the handle's
 * own 16-bit copies).  It only reads the workspace: any number of calls, the same workspace gives the same bits.  The position gradient
 * is that of the fp32 trilinear blend whatever blend_fp16 says, the aabb selector contributes nothing.  `positions` is not read (the
 * workspace holds them normalised) and may be NULL; `directions` [n,3] may be NULL when d_directions is.
 * Both outputs NULL, n < 0, loss_scale <= 0 or d_directions without directions return MNF_ERR_INVALID, n == 0 returns MNF_OK, a
 * workspace smaller than mnf_field_train_workspace_bytes(f, n) returns MNF_ERR_WORKSPACE: all before any HIP call.  Profile label:
 * "field_input_grad".  Enqueues on `stream` and does not synchronise. */
int mnf_field_backward_inputs(mnf_field_t f, const float *positions, const float *directions, int64_t n,
                              void *workspace, int64_t workspace_bytes, float loss_scale,
                              float *d_positions, float *d_directions, mnf_stream_t stream);
/* The same tcnn input gradient carried on to the rays of packed samples grouped by ray (the closure of utils.py:122-137,
 * positions = origins + dirs * (t_starts + t_ends) / 2, directions = dirs): g_rays_o[r] = sum_s d_positions[s],
 * g_rays_d[r] = sum_s ((t_starts[s] + t_ends[s]) / 2 * d_positions[s] + d_directions[s]) over the samples
 * chunk_starts[r] .. chunk_starts[r] + chunk_cnts[r] - 1 of ray r.  One wave per ray: lane L adds samples L, L + 64, ... in index
 * order, the 64 partial sums are added by a fixed butterfly; fp32, no atomics, rays without samples get exact zeros.  d_directions may
 * be NULL (position term only); one of g_rays_o / g_rays_d [n_rays,3] may be NULL.  Enqueues on `stream` and does not synchronise. */
int mnf_ray_input_gradients(const float *d_positions, const float *d_directions, const float *t_starts, const float *t_ends,
                            const int64_t *chunk_starts, const int64_t *chunk_cnts, int32_t n_rays, int64_t n_samples,
                            float *g_rays_o, float *g_rays_d, mnf_stream_t stream);

/* ---------------------------------------------------------------- one training iteration's forward + loss + backward
 * scripts/pipeline.py:472-518 for one model as ONE call: the train render `render_image_with_occgrid_with_depth_guide`
 * (perception/models/utils.py:63-219: occupancy sampling with stratified near planes, density pre-pass and visibility filter,
 * occ_grid.py:80-238; then sem_rendering, utils.py:362-461), the loss 10 smooth_l1(rgb) + smooth_l1(depth) / 5 + CE(sem) / 2
 * (pipeline.py:506-511) and its backward to the three flat parameter-gradient vectors g_base / g_head / g_sem (overwritten).
 * Not included, as in the reference they belong to the caller: occupancy refresh (mnf_update_occupancy), NaN guard
 * (mnf_count_nan), optimizer (mnf_adam_step / mnf_adam_step_guarded).  losses (device, 4 floats): total, rgb, depth, semantic
 * terms (un-weighted means).
 * NO stream synchronisation: the sample counts stay on the device.  counts_dev (DEVICE, 4 x int64): [0] marched samples, [1] surviving
 * samples (= the reference's n_rendering_samples), [2] samples of the longest ray, [3] status bits: 1 marched > max_marched, 2 a ray
 * longer than a scratch row (use the two-pass sampler), 4 surviving > max_kept, 8 a class id outside [0, C) (F.cross_entropy's device
 * assert), 16 no sample survived (the reference `continue`s, pipeline.py:491), 32 (mnf_train_render_backward / _backward_rays only) a non-finite incoming gradient.  skip_dev (DEVICE int32): set to 0, then raised for
 * every status bit: with it non-zero the gradients are zero / must not be applied (mnf_adam_step_guarded reads it).  The caller
 * bounds the sample counts (max_marched, max_kept), provides mnf_train_step_workspace_bytes(), reads counts_dev when it wants
 * to and retries with larger bounds after bits 1 / 4.
 * Stratified near planes: near + U[0,1) * render_step_size per ray from Philox4x32-10 (counter (ray, 0, 7, 0), key = seed). */
typedef struct {
    uint32_t struct_size;     /* sizeof(mnf_train_opts) */
    float near_plane, far_plane, render_step_size, cone_angle, alpha_thre, early_stop_eps;   /* utils.py:63-76 / occ_grid.py:80-96 */
    float render_bkgd[3];
    float loss_scale;         /* fp16 activation-gradient scale of the backward (tcnn: 128) */
    int32_t stratified;       /* occ_grid.py:187-189 (radiance_field.training) */
    uint64_t seed;
    const float *render_bkgd_dev;   /* optional: 3 device floats used instead of render_bkgd (pipeline.py:437 draws the colour on
                                       the GPU: no host copy of it is needed) */
    int32_t deterministic;          /* 0 (default): gradients accumulate with float atomics (the reference's index_add_ / tcnn atomics: the
                                       result depends on arrival order in the last bits).  1: bitwise reproducible — the hash-table gradient
                                       accumulates in 64-bit fixed point (integer atomics), the weight gradients' partial sums are added in
                                       a fixed order.  Same kernels otherwise; used for stand-in scenes that must come out the same on
                                       every box (apnrf_amd.standin) and for regression tests. */
    int32_t n_levels;               /* occupancy levels (0 or 1: one): binaries [n_levels,X,Y,Z], occs [n_levels * cells], aabb_host n_levels x 6 floats,
                                       bitgrid [n_levels][ceil(cells / 32)]; the field's aabb is the largest level's (pipeline.py:167-172) */
    struct mnf_presample_s *presampled;   /* optional (NULL: march inside the step): a mnf_train_presample of exactly these rays, options and grid, see below */
} mnf_train_opts;
/* The parameter-independent head of a training iteration, ahead of time.  The march of a batch (occ_grid.py:181-208: stratified near planes, the alpha
 * threshold from the grid's mean occupancy, traverse_grids, per-ray offsets) reads the rays and the occupancy grid but not the model: the reference runs it inside
 * every iteration, where one lane per ray leaves most of the chip idle for 0.2 ms.  mnf_train_presample runs it for the NEXT batch on a library-owned
 * side stream, forked from `stream` as it is at the call — call it BEFORE enqueuing the current iteration and it marches beside that iteration's kernels —
 * and mnf_train_step adopts the result when opts->presampled names the handle (it waits for the march on its own stream; same rays / options / seed / grid
 * pointers required, MNF_ERR_INVALID otherwise; one use).  Results are bit-identical to marching inside the step.  The caller keeps rays, grid and `workspace`
 * (mnf_train_presample_workspace_bytes(n_rays, max_marched) device bytes; max_marched: the adopting step's bound, checked there — the march's guard and the packing of its samples run in the presample too) untouched until the adopting step has been enqueued, and must not refresh the occupancy grid in
 * between without mnf_presample_wait (then simply do not pass the handle: the step marches itself).
 * Replaces nothing in the reference's call list: a scheduling entry point (the data loader's "next batch" prefetch applied to the sampler). */
typedef struct mnf_presample_s *mnf_presample_t;
int mnf_presample_create(mnf_presample_t *out);
void mnf_presample_destroy(mnf_presample_t p);
int64_t mnf_train_presample_workspace_bytes(int32_t n_rays, int64_t max_marched);
int mnf_train_presample(mnf_presample_t p, const uint8_t *binaries, const uint32_t *bitgrid, const float *occs, int32_t res_x, int32_t res_y,
                        int32_t res_z, const float *aabb_host, const float *rays_o, const float *rays_d, int32_t n_rays,
                        const mnf_train_opts *opts, int64_t max_marched, void *workspace, int64_t workspace_bytes, mnf_stream_t stream);
/* make `stream` wait for the handle's march (no-op if none was launched) */
int mnf_presample_wait(mnf_presample_t p, mnf_stream_t stream);

int64_t mnf_train_step_workspace_bytes(mnf_field_t f, int32_t n_rays, int64_t max_marched, int64_t max_kept);
int mnf_train_step(mnf_field_t f, const uint8_t *binaries, const uint32_t *bitgrid, const float *occs, int32_t res_x, int32_t res_y,
                   int32_t res_z, const float *aabb_host, const float *rays_o, const float *rays_d, int32_t n_rays,
                   const float *target_rgb, const float *target_depth, const int64_t *target_sem, const mnf_train_opts *opts,
                   float *g_base, float *g_head, float *g_sem, float *losses, int64_t *counts_dev, int32_t *skip_dev, int64_t max_marched,
                   int64_t max_kept, void *workspace, int64_t workspace_bytes, mnf_stream_t stream);

/* The same iteration cut at its loss, for a caller whose loss is not the one mnf_train_step computes (the reference's own loss lines kept in torch, masked
 * depth, other weights, a term on the opacity, label smoothing): mnf_train_render_forward is pipeline.py:472-489 — the train render
 * `render_image_with_occgrid_with_depth_guide`, utils.py:63-219 — and mnf_train_render_backward is what `loss.backward()` (pipeline.py:518) does below the
 * four rendered planes.  Both launch exactly the kernels mnf_train_step launches on its side of the loss, in the same order, so rendered values, sample
 * counts and gradients are the step's.  Arguments as mnf_train_step's; opts->presampled must be NULL (MNF_ERR_INVALID otherwise).
 *
 * mnf_train_render_forward writes rgb [n_rays,3], acc [n_rays], depth [n_rays], sem [n_rays,C] (ray-major, dense) and fills counts_dev / skip_dev as the step
 * does (status bits 1, 2, 4, 16).  It touches no gradient vector.  When a guard fires or no sample survives the outputs are still defined: the background
 * colour, acc 0, depth 0, sem 0.  `sem` may be NULL for a field without semantic classes (C == 0), and only then.
 *
 * mnf_train_render_backward takes dL/d(rgb, acc, depth, sem) as the caller's autograd delivers them: each pointer may be NULL (= zero) and comes with its
 * row stride (and, for rgb / sem, column stride) in ELEMENTS — element (r, c) is read at g[r * row_stride + c * col_stride]; stride 0 (an expanded scalar)
 * and transposed views are fine, no dense copy is needed.  g_base / g_head / g_sem_params are OVERWRITTEN, not accumulated.  counts_dev / skip_dev are the
 * forward's: with the skip flag already raised the gradients come out zero; a non-finite incoming value raises status bit 32 and the skip flag and the
 * gradients come out zero as well (pipeline.py:520-529 decided on the device: mnf_adam_step_guarded then leaves the parameters alone).
 *
 * Contract: every bit of per-call state lives in `workspace` (mnf_train_step_workspace_bytes(f, n_rays, max_marched, max_kept) bytes, the same n_rays and
 * bounds in both calls).  Between a forward and its backward the workspace, the field's loaded weights (no mnf_field_set_params / optimizer step on `f`), the
 * options and — if used — the three floats behind opts->render_bkgd_dev must stay unchanged; the occupancy grid and the ray origins are not read again, and the
 * ray directions only by mnf_train_render_backward_rays (below), which is handed the forward's array again.  Other
 * forwards and backwards of the same field with OTHER workspaces may run in between (the deterministic mode's scratch on the field handle is only touched
 * inside a backward).  One backward per forward: the backward overwrites workspace state. */
int mnf_train_render_forward(mnf_field_t f, const uint8_t *binaries, const uint32_t *bitgrid, const float *occs, int32_t res_x, int32_t res_y,
                             int32_t res_z, const float *aabb_host, const float *rays_o, const float *rays_d, int32_t n_rays,
                             const mnf_train_opts *opts, float *rgb, float *acc, float *depth, float *sem, int64_t *counts_dev, int32_t *skip_dev,
                             int64_t max_marched, int64_t max_kept, void *workspace, int64_t workspace_bytes, mnf_stream_t stream);
int mnf_train_render_backward(mnf_field_t f, int32_t n_rays, const mnf_train_opts *opts, const float *g_rgb, int64_t g_rgb_row_stride,
                              int64_t g_rgb_col_stride, const float *g_acc, int64_t g_acc_row_stride, const float *g_depth, int64_t g_depth_row_stride,
                              const float *g_sem, int64_t g_sem_row_stride, int64_t g_sem_col_stride, float *g_base, float *g_head, float *g_sem_params,
                              int64_t *counts_dev, int32_t *skip_dev, int64_t max_marched, int64_t max_kept, void *workspace, int64_t workspace_bytes,
                              mnf_stream_t stream);
/* mnf_train_render_backward for a caller who differentiates with respect to the RAYS (a pose refiner: `loss.backward()`, pipeline.py:518, behind the train
 * render of utils.py:63-219 with `rays.origins` / `rays.viewdirs` requiring a gradient): the same backward, then ONE more kernel that goes from what it left
 * in the workspace — dX, the head's dZr1 rows, the kept samples' normalised positions, distances and per-ray runs — straight to
 *   g_rays_o[r] = sum_s d_position[s],   g_rays_d[r] = sum_s (t_starts[s] + t_ends[s]) / 2 * d_position[s]  +  J_SH(rays_d[r])^T sum_s W1_head[:, 0:16]^T dZr1[s]
 * over the kept samples s of ray r ([n_rays,3] fp32, OVERWRITTEN; one of the two may be NULL).  The per-sample arithmetic is mnf_field_backward_inputs', the sum
 * mnf_ray_input_gradients' (one wave per ray, lane L the samples L, L + 64, ..., a fixed butterfly): no atomics, the same inputs give the same bits; rays
 * without kept samples get exact zeros.  The sample set is a constant of the render (it does not move with the rays), t_starts / t_ends and the background
 * colour get no gradient.  Profile label of the added kernel: "train_render_ray_grad".
 * g_base / g_head / g_sem_params: all three given — exactly mnf_train_render_backward's launches, then the kernel; all three NULL — the parameters are FROZEN:
 * nothing is filled, the output gradients and the backward-data kernel run, the weight gradients, the hash-table scatter and their side streams do not.
 * rays_d [n_rays,3] is the array the forward was given, unchanged; it may be NULL only when g_rays_d is.  With the skip flag raised (the forward's verdict, or
 * status bit 32 from a non-finite incoming gradient) the ray gradients are exact zeros, as the parameter gradients are.
 * MNF_ERR_INVALID before any HIP call: both ray outputs NULL, one or two of the three parameter pointers NULL, g_rays_d without rays_d, opts->presampled set, a
 * wrong struct_size, n_rays / max_marched / max_kept <= 0; MNF_ERR_WORKSPACE: a NULL or short workspace.  One backward per forward, as above.  Enqueues on
 * `stream` and does not synchronise. */
int mnf_train_render_backward_rays(mnf_field_t f, int32_t n_rays, const mnf_train_opts *opts, const float *rays_d, const float *g_rgb,
                                   int64_t g_rgb_row_stride, int64_t g_rgb_col_stride, const float *g_acc, int64_t g_acc_row_stride, const float *g_depth,
                                   int64_t g_depth_row_stride, const float *g_sem, int64_t g_sem_row_stride, int64_t g_sem_col_stride, float *g_base,
                                   float *g_head, float *g_sem_params, float *g_rays_o, float *g_rays_d, int64_t *counts_dev, int32_t *skip_dev,
                                   int64_t max_marched, int64_t max_kept, void *workspace, int64_t workspace_bytes, mnf_stream_t stream);

/* ---------------------------------------------------------------- fused test-mode renderers */

typedef struct {
    uint32_t struct_size;    /* sizeof(mnf_render_opts), see MNF_INIT */
    float near_plane;        /* utils.py:563 */
    float far_plane;         /* utils.py:564 */
    float render_step_size;  /* utils.py:565 */
    float cone_angle;        /* utils.py:567 */
    float alpha_thre;        /* utils.py:568 */
    float early_stop_eps;    /* utils.py:569 */
    float render_bkgd[3];    /* utils.py:566 */
    int32_t max_samples;     /* utils.py:557 */
    int32_t probabilistic;   /* 0: render_image_with_occgrid_test, 1: render_probablistic_image_with_occgrid_test */
    int32_t rays_per_view;   /* rays of one reference call; n_rays must be a multiple of it.  Each group of
                                rays_per_view consecutive rays is rendered exactly as one call of the reference
                                function (its own n_alive / n_samples round schedule, utils.py:667-672). */
    int32_t sync_every;      /* host checks the device "all views finished" flag every this many rounds
                                (stream sync); 0 = never (all ceil(max_samples/min_samples) rounds are enqueued) */
    const int32_t *view_order; /* optional (NULL = identity): device permutation of 0..rays_per_view-1, the order in which the
                                rays of every view are marched and packed into the field kernel's 64-column tiles.  Results
                                are per ray and do not depend on it; rays that are neighbours in the image should be
                                neighbours in this order (e.g. 8x8 pixel blocks instead of one-pixel-high strips) so that
                                a tile's samples share hash-table lines. */
    const uint32_t *bitgrid; /* optional (NULL = packed from `binaries` at the start of the call): the bit-packed form of
                                `binaries` that mnf_occ_binarize / mnf_pack_bitgrid maintain (bit c & 31 of word c >> 5;
                                [n_levels][ceil(cells / 32)] words) */
    int32_t n_levels;        /* occupancy levels (occ_grid.py:37-55: level l covers the roi enlarged 2^l times); 0 or 1 = one level.
                                With n_levels > 1 `binaries` is [n_levels,X,Y,Z], `aabb_host` holds n_levels x 6 floats
                                (estimator.aabbs) and a ray's segments are taken level by level as grid.cu:125-151 does (<= 4 levels) */
} mnf_render_opts;

/* bytes of workspace mnf_render_test needs for n_rays rays */
int64_t mnf_render_workspace_bytes(int64_t n_rays, int32_t rays_per_view);

/* render_image_with_occgrid_test (perception/models/utils.py:555-779) and
 * render_probablistic_image_with_occgrid_test (utils.py:782-1032).
 * binaries [L,X,Y,Z] u8, aabb_host[6 L] = estimator.aabbs, L = opts->n_levels (0 or 1: one level; <= 4).
 * Outputs: rgb [n,3], acc [n,1], depth [n,1], sem [n,C]; rgb_var [n,3], depth_var [n,1] (probabilistic only,
 * may be NULL otherwise); total_samples: TWO int64 (device): [0] = the reference's total_samples (samples kept
 * after the alpha threshold, utils.py:757), [1] = samples evaluated by the field (all marched samples).
 * Synchronises the stream only as sync_every asks. */
int mnf_render_test(mnf_field_t f, const uint8_t *binaries, int32_t res_x, int32_t res_y, int32_t res_z,
                    const float *aabb_host, const float *rays_o, const float *rays_d, int64_t n_rays,
                    const mnf_render_opts *opts,
                    float *rgb, float *acc, float *depth, float *sem, float *rgb_var, float *depth_var,
                    int64_t *total_samples, void *workspace, int64_t workspace_bytes, mnf_stream_t stream);

/* Several independent render calls advancing side by side (the members of an ensemble rendering the same candidate views,
 * pipeline.py:697-711 called once per member; or groups of views of one pose list, habitat_to_data.py:304-549): every job is what
 * one mnf_render_test call is, with its own field / grid / rays / outputs / workspace; job 0 runs on `stream`, the others on
 * streams of the library that fork from and join `stream`.  While one job's short kernels leave compute units idle the others'
 * launches use them.  Results are those of separate mnf_render_test calls, bit for bit.  `opts->bitgrid` is ignored (per job). */
typedef struct {
    uint32_t struct_size;         /* sizeof(mnf_render_job) in EVERY element of the array, see MNF_INIT */
    mnf_field_t field;
    const uint8_t *binaries;      /* [L,X,Y,Z] u8, L = opts->n_levels */
    const uint32_t *bitgrid;      /* optional packed form of `binaries` (see mnf_render_opts.bitgrid) */
    const float *rays_o, *rays_d; /* [n_rays,3] */
    int64_t n_rays;               /* a multiple of opts->rays_per_view; 0 = nothing to do */
    float *rgb, *acc, *depth, *sem, *rgb_var, *depth_var;
    int64_t *total_samples;       /* 2 x int64 (device) */
    void *workspace;              /* mnf_render_workspace_bytes(n_rays, rays_per_view), not shared between jobs */
    int64_t workspace_bytes;
} mnf_render_job;
int mnf_render_jobs(const mnf_render_job *jobs_host, int32_t n_jobs, int32_t res_x, int32_t res_y, int32_t res_z,
                    const float *aabb_host, const mnf_render_opts *opts, mnf_stream_t stream);

/* ---------------------------------------------------------------- planner hand-off
 * The only perception artefact the planner reads (scripts/pipeline.py:1043-1049, planning/planning_funcs.py:243-261):
 * binaries [n_members,X,Y,Z] u8 (the ensemble's `estimator.binaries[0]`), sliced at height index y_slice (8 in the
 * reference), merged over members and dilated by the 3x3 box with symmetric boundary -> out_map [X,Z] int32 (1 = blocked).
 * The caller clears the cells around the vehicle (planning_funcs.py:262-266) on the host. */
int mnf_planner_map(const uint8_t *binaries, int32_t n_members, int32_t res_x, int32_t res_y, int32_t res_z,
                    int32_t y_slice, int32_t *out_map, mnf_stream_t stream);

/* Optional in-library kernel timing for bench.py's roofline figures: between begin and end the library brackets its main
 * launches with hipEvent pairs on the launch stream, grouped by label: "field_render" (the fused field kernel of
 * mnf_render_test), "field_density", "field_forward", "field_train_forward", "dgrad", "wgrad", "hash_scatter", "field_input_grad",
 * "composite_train_forward", "composite_train_backward", "sample_rays", "eval_views", "frames_views", "score_view_maps".  mnf_profile_end synchronises the events, sums
 * the milliseconds per label and returns the "field_render" totals; mnf_profile_query reads any label afterwards.
 * Process-wide (backward passes run on torch's autograd thread).  Not part of the reference surface. */
int mnf_profile_begin(void);
int mnf_profile_end(double *field_ms_host, int64_t *launches_host);
int mnf_profile_query(const char *label_host, double *ms_host, int64_t *launches_host);

/* ---------------------------------------------------------------- predictive-information scorer */

/* scripts/pipeline.py:727-781 on device.  Inputs are the renders of n_members ensemble members for the
 * same n_views views of n_pix pixels: member-major arrays rgb_var [M,V,P,3], depth_var [M,V,P], acc [M,V,P],
 * sem [M,V,P,C] f32.  Output terms [V,4] f64 = per-view means of the rgb / depth / semantic / occupancy
 * predictive-information terms (un-weighted); the trajectory score is
 * mean_v(t0 + t1 + 3*t2 + 2*t3) (pipeline.py:775-781). */
int mnf_score_views(const float *rgb_var, const float *depth_var, const float *acc, const float *sem,
                    int32_t n_members, int32_t n_views, int32_t n_pix, int32_t n_classes,
                    double *terms, mnf_stream_t stream);

/* scripts/pipeline.py:674-781 for one trajectory as ONE call: candidate poses (c2w [n_views,3,4] f32, device) -> the
 * sub-sampled rays of every view (pix_idx [n_pix] int64, device: the np.round(np.linspace) pixels of habitat_to_data.py:462-467)
 * -> probabilistic renders by every ensemble member (fields_host / binaries_host / bitgrids_host: HOST arrays of n_members
 * handles / device pointers; bitgrids_host or its entries may be NULL) -> per-view terms [n_views,4] f64 as mnf_score_views. */
int64_t mnf_score_poses_workspace_bytes(int32_t n_members, int32_t n_views, int32_t n_pix, int32_t n_classes);
int mnf_score_poses(const mnf_field_t *fields_host, const uint8_t *const *binaries_host, const uint32_t *const *bitgrids_host,
                    int32_t n_members, int32_t res_x, int32_t res_y, int32_t res_z, const float *aabb_host, const float *c2w,
                    int32_t n_views, int32_t width, int32_t height, float focal, const int64_t *pix_idx, int64_t n_pix,
                    const mnf_render_opts *opts, double *terms, void *workspace, int64_t workspace_bytes, mnf_stream_t stream);

/* ---------------------------------------------------------------- predictive-information maps */

/* scripts/pipeline.py:727-774 on device with the four terms KEPT PER PIXEL (the reference forms them as [V,h,w] arrays and collapses
 * each with np.mean at :735 / :746 / :760 / :773; a caller who wants to see where a view carries information redoes them on the host
 * from six float64 stacks, 272 bytes per pixel at M = 2, C = 29).  Inputs as mnf_score_views': the probabilistic renders of n_members
 * ensemble members for the same n_views views of n_pix pixels, member-major rgb_var [M,V,P,3], depth_var [M,V,P], acc [M,V,P],
 * sem [M,V,P,C] f32 (any 4-byte alignment).  Per pixel, in double from the widened fp32 inputs, k = 2 pi e, members added in order:
 *   [0] rgb    mean over the three channels of  log(k (sum_m x) / 2 + 1e-4) / 2 - (1 / M) sum_m log(k x_m + 1e-4) / 2
 *              (the / 2 under the first logarithm is the reference's, whatever M is: pipeline.py:733)
 *   [1] depth  the same expression on the one channel of depth_var
 *   [2] sem    H(mean_m p_m) - mean_m H(p_m), p_m the softmax of member m's logits (maximum subtracted),
 *              H(q) = -sum_k (q_k + 1e-4) log(q_k + 1e-4)
 *   [3] occ    B(mean_m a_m) - mean_m B(a_m), B(a) = -(a + 1e-4) log(a + 1e-4) - (1 - a + 1e-4) log(1 - a + 1e-4)
 * NaN and inf propagate as they do in numpy.  Outputs (each may be NULL = skipped, at least one must not be; no byte outside an
 * output's extent is written):
 *   terms [V,4] f64   the per-view means, un-weighted, in mnf_score_views' column order; 8-byte aligned;
 *   maps [V,P,4] f64  the four terms of every pixel; 8-byte aligned (16-byte aligned bases are stored with 16-byte stores);
 *   heat8 [V,P,4] u8  sat8(((x - lo_k) / (hi_k - lo_k)) * 255.0) in float64 with exactly those operations in that order,
 *                     sat8 as mnf_frames_views' (clamp to [0, 255], round to nearest even, NaN -> 0), lo = heat_lo_host[4] and
 *                     hi = heat_hi_host[4] HOST doubles, hi < lo reverses a ramp; 4-byte aligned.  A colour look-up table is the
 *                     caller's: index it with these bytes.
 * No atomics: the same inputs give the same bits, and a view's rows depend on that view's data, P, M and C only, not on n_views or
 * on its position in the call.  workspace: mnf_score_view_maps_workspace_bytes(V, P, C) bytes, 8-byte aligned (per-workgroup partial
 * sums; read only when terms is asked for).  Argument errors (a size < 1, all three outputs NULL, heat8 without its ranges, hi == lo or
 * a non-finite range, a misaligned maps / heat8, a workspace that is too small, more than 65535 views) return MNF_ERR_INVALID,
 * n_members or n_classes above the two maxima below MNF_ERR_UNSUPPORTED, both before any HIP call; n_views == 0 returns MNF_OK.
 * Profile label: "score_view_maps".  Enqueues on `stream` and does not synchronise. */
#define MNF_SCORE_MAPS_MAX_MEMBERS 64
#define MNF_SCORE_MAPS_MAX_CLASSES 1024
int64_t mnf_score_view_maps_workspace_bytes(int32_t n_views, int64_t n_pix, int32_t n_classes);
int mnf_score_view_maps(const float *rgb_var, const float *depth_var, const float *acc, const float *sem, int32_t n_members,
                        int32_t n_views, int64_t n_pix, int32_t n_classes, double *terms, double *maps, uint8_t *heat8,
                        const double *heat_lo_host, const double *heat_hi_host, void *workspace, int64_t workspace_bytes,
                        mnf_stream_t stream);

/* ---------------------------------------------------------------- ensemble-disagreement scorer */

/* scripts/pipeline.py:861-882 (`trajector_uncertainty`) on device.  Inputs are the plain renders of n_members ensemble members for
 * the same n_views views of n_pix pixels: member-major arrays rgb [M,V,P,3], depth [M,V,P], acc [M,V,P] (only member 0 is read,
 * pipeline.py:869) and sem [S,V,P,C] f32, the class logits of the first n_sem_members = S members, 1 <= S <= M (S = 1 is the
 * reference; S > 1 averages the entropy over those members as np.mean(sem_entropy, axis=(0,2,3)) would).
 * Output terms [V,4] f64, the four clipped rows of pipeline.py:875-882, per view:
 *   [0] clip(4000 * mean_p mean_ch var_m(rgb), 0, 100)            [1] clip(50 * mean_p var_m(depth), 0, 100)
 *   [2] mean_p clip(1 / (acc_0 + 1e-4) - 1, 0, 10000)             [3] clip(50 * mean_{s,p} H, 0, 100)
 * with H = -sum_k p_k log(p_k + 1e-10), p the softmax of the logits (maximum subtracted), and var the population variance (np.var)
 * taken in two passes (mean over the members, then the mean squared deviation).  All arithmetic is double from the widened fp32
 * inputs; NaN propagates as through np.clip.  No atomics: the same inputs give the same bits, and a view's row depends on that
 * view's data, P, M, S and C only, not on n_views or on its position in the call.  The stacks need 4-byte alignment only.
 * workspace: mnf_score_ensemble_views_workspace_bytes(V, P, C) bytes, 8-byte aligned (per-workgroup partial sums).  Argument errors
 * (n_members < 1, S outside [1, M], a workspace that is too small) return MNF_ERR_INVALID, n_members or n_classes above the two
 * maxima below MNF_ERR_UNSUPPORTED, both before anything is enqueued; n_views == 0 returns MNF_OK.  Enqueues on `stream` and does
 * not synchronise. */
#define MNF_SCORE_ENSEMBLE_MAX_MEMBERS 64
#define MNF_SCORE_ENSEMBLE_MAX_CLASSES 1024
int64_t mnf_score_ensemble_views_workspace_bytes(int32_t n_views, int64_t n_pix, int32_t n_classes);
int mnf_score_ensemble_views(const float *rgb, const float *depth, const float *acc, const float *sem, int32_t n_members,
                             int32_t n_sem_members, int32_t n_views, int64_t n_pix, int32_t n_classes, double *terms,
                             void *workspace, int64_t workspace_bytes, mnf_stream_t stream);

/* scripts/pipeline.py:807-882 for one trajectory as ONE call, the plumbing of mnf_score_poses: poses (c2w [n_views,3,4] f32, device)
 * -> the sub-sampled rays of every view (pix_idx [n_pix] int64, device) -> every member's plain render (not probabilistic, black
 * background, opts->max_samples per round: what Dataset.render_image_from_pose does with 1024) as a job of mnf_render_jobs, laid out
 * member-major in the workspace -> mnf_score_ensemble_views with S = 1 -> terms [n_views,4] f64.  opts->probabilistic and
 * opts->render_bkgd are overridden. */
int64_t mnf_score_trajectory_workspace_bytes(int32_t n_members, int32_t n_views, int32_t n_pix, int32_t n_classes);
int mnf_score_trajectory(const mnf_field_t *fields_host, const uint8_t *const *binaries_host, const uint32_t *const *bitgrids_host,
                         int32_t n_members, int32_t res_x, int32_t res_y, int32_t res_z, const float *aabb_host, const float *c2w,
                         int32_t n_views, int32_t width, int32_t height, float focal, const int64_t *pix_idx, int64_t n_pix,
                         const mnf_render_opts *opts, double *terms, void *workspace, int64_t workspace_bytes, mnf_stream_t stream);

/* ---------------------------------------------------------------- held-out view evaluation */

/* The error metrics of scripts/pipeline.py:550-613 (per test image: F.cross_entropy on the [H*W, C] logits, F.mse_loss on rgb and
 * depth, PSNR, each behind a blocking .item(), every plane copied to the host) and the label image of :1011 (np.argmax over a float64
 * [H, W, C] host stack), as one pass over the finished renders of n_views views of n_pix pixels: rgb [V,P,3], depth [V,P],
 * sem [V,P,C] f32.  Ground truth is read from the dataset's own storage, either layout mnf_gather_pixels accepts (gt_images u8
 * [N,pixels_per_image,3]; gt_depths f32, or f16 with depth_is_f16; gt_semantics int64, or u8 with sem_is_u8): pixel p of view v is
 * pixel image_ids[v] * pixels_per_image + (pix_idx ? pix_idx[p] : p) of the storage (image_ids [V], pix_idx [P] or NULL, int64).
 * Ground-truth rgb is (float)u8 / 255.0f as mnf_gather_pixels computes it; differences, squares, sums, the log-sum-exp (maximum
 * subtracted) and the logarithms are double.  The predicted class is the first maximal logit (torch.argmax / np.argmax).
 * metrics [V,8] f64, per view: [0] rgb MSE over P*3, [1] PSNR = -10 ln(mse) / ln(10) (+inf at mse 0), [2] depth MSE, [3] semantic
 * cross-entropy and [4] pixel accuracy, both over the pixels whose label lies in [0, C), [5] the number of those pixels, [6] the
 * number of pixels with a label outside [0, C) (left out of [3], [4] and the matrix), [7] 0 (reserved).  A view without a valid
 * label has NaN in [3] and [4]; NaN / inf in a render propagate as they do in torch.
 * Optional outputs (NULL = skip): confusion [C,C] int64, rows = ground-truth class, columns = predicted class, summed over the views
 * of the call and WRITTEN, not accumulated into (counted in an LDS histogram per workgroup for C <= 64, with global integer atomics
 * directly above that); pred_labels [V,P] u8, the argmax map (needs C <= 256).
 * No floating-point atomics: the same inputs give the same bits, and a view's row does not depend on the other views of the call.
 * workspace: mnf_eval_views_workspace_bytes(V, P, C) bytes, 8-byte aligned (per-workgroup partial sums).  Argument errors return
 * MNF_ERR_INVALID (a workspace that is too small included) before anything is enqueued; C > 10239 returns MNF_ERR_UNSUPPORTED;
 * n_views == 0 returns MNF_OK.  Enqueues on `stream` and does not synchronise. */
int64_t mnf_eval_views_workspace_bytes(int32_t n_views, int64_t n_pix, int32_t n_classes);
int mnf_eval_views(const float *rgb, const float *depth, const float *sem, int32_t n_views, int64_t n_pix, int32_t n_classes,
                   const uint8_t *gt_images, const void *gt_depths, int32_t depth_is_f16, const void *gt_semantics, int32_t sem_is_u8,
                   int64_t pixels_per_image, const int64_t *image_ids, const int64_t *pix_idx,
                   double *metrics, int64_t *confusion, uint8_t *pred_labels,
                   void *workspace, int64_t workspace_bytes, mnf_stream_t stream);

/* The structural similarity (SSIM, Wang et al. 2004) that belongs next to the PSNR of scripts/pipeline.py:550-613 (the reference imports
 * skimage at :20; a caller who wants the number copies the float planes of every view to the host and filters them there), as one pass
 * over the finished planes of n_views views of height x width pixels of `channels` channels: pred [V,H,W,K] f32 against target_f32
 * [V,H,W,K] f32, or against target_u8, the dataset's image storage [N,pixels_per_image,3] u8 (view v is image image_ids[v], int64 on
 * the device; needs K = 3 and pixels_per_image == H * W; a stored byte is (float)u8 / 255.0f as mnf_gather_pixels computes it).
 * Exactly one of the two targets is given.  The quantity is what skimage.metrics.structural_similarity(gaussian_weights=True,
 * sigma=1.5, use_sample_covariance=False, data_range=L, channel_axis=-1) returns after its border crop, over the VALID windows only,
 * in double from the widened fp32 inputs:
 *   g[i] = exp(-0.5 ((i - 5) / 1.5)^2), i = 0 .. 10, normalised to sum 1; the window is g (x) g, applied separably, rows (along W)
 *   first, then columns, taps added in index order, no padding: outputs exist for the (H - 10) x (W - 10) window centres only;
 *   per channel the five filtered planes mx, my, E[xx], E[yy], E[xy]; vx = E[xx] - mx mx, vy likewise, cxy = E[xy] - mx my;
 *   S_c = ((2 mx my + C1) (2 cxy + C2)) / ((mx mx + my my + C1) (vx + vy + C2)), C1 = (k1 L)^2, C2 = (k2 L)^2, L = data_range
 *   (k1 = 0.01, k2 = 0.03 are the usual constants).
 * Outputs: ssim [V] f64 = the sum of S_c over centres and channels / ((H - 10) (W - 10) K); map [V,H-10,W-10] f64 or NULL =
 * (S_0 + ... + S_{K-1}) / K per centre; both 8-byte aligned, no byte outside them is written.  Identical images give exactly 1.0 at
 * every centre.  NaN / inf propagate as they do in numpy: a NaN pixel makes exactly the <= 11 x 11 centres whose window covers it NaN.
 * No floating-point atomics: the same inputs give the same bits, and a view's bits depend on that view's data, H, W and K only, not
 * on n_views or on its position in the call.  The f32 planes need 4-byte alignment only; nothing outside the planes is read.
 * workspace: mnf_ssim_views_workspace_bytes(V, H, W, K) bytes, 8-byte aligned (per-workgroup partial sums).  Argument errors (H or
 * W < 11, K outside 1 .. 4, both or neither target, a u8 target with K != 3 or pixels_per_image != H * W, a non-finite or
 * non-positive data_range, a non-finite or negative k1 / k2, ssim NULL, a misaligned map, a workspace that is too small, more than
 * 65535 views) return MNF_ERR_INVALID before any HIP call; n_views == 0 returns MNF_OK.  Profile label: "ssim_views".  Enqueues on
 * `stream` and does not synchronise. */
#define MNF_SSIM_WINDOW 11
#define MNF_SSIM_SIGMA 1.5
#define MNF_SSIM_MAX_CHANNELS 4
int64_t mnf_ssim_views_workspace_bytes(int32_t n_views, int32_t height, int32_t width, int32_t channels);
int mnf_ssim_views(const float *pred, const float *target_f32, const uint8_t *target_u8, const int64_t *image_ids,
                   int64_t pixels_per_image, int32_t n_views, int32_t height, int32_t width, int32_t channels,
                   double data_range, double k1, double k2, double *ssim, double *map,
                   void *workspace, int64_t workspace_bytes, mnf_stream_t stream);

/* ---------------------------------------------------------------- 8-bit frames of finished renders */

/* The frame conversion of scripts/pipeline.py:976-1023 (per rendered pose: np.float32(rgb * 255), np.clip(dep * 25, 0, 255), acc * 255,
 * np.argmax over the float64 [h, w, C] stack, the palette indexed by the label, cv2.cvtColor to BGR, cv2.imwrite narrowing to 8 bits) and
 * of visualization/vis_nerf_habitat.py:142-179 (clip(depth / 10, 0, 1) * 255), as one pass over the finished planes of n_views views of
 * n_pix pixels: rgb [V,P,3], depth [V,P], acc [V,P], sem [V,P,C] f32 (any 4-byte alignment).  With
 *   sat8(x) = x clamped to [0, 255], rounded to nearest with ties to even, NaN -> 0, +inf -> 255, -inf -> 0
 * the outputs (each may be NULL = skipped; each may start at ANY byte; no byte outside its extent is written) are
 *   rgb8 [V,P,3] = sat8(x * 255.0f), multiplied and rounded in float32 (what np.float32(float64(x) * 255) is);
 *   occ8 [V,P]   = sat8((double)acc * 255.0);
 *   dep8 [V,P]   = sat8(clip(((double)d * depth_mul) / depth_div, 0, depth_clip_hi) * depth_gain) in float64, clip = np.clip (a NaN stays
 *                  a NaN and becomes 0): (25, 1, 255, 1) is the pipeline's mapping, (1, 10, 1, 255) the viewer's;
 *   labels [V,P] = the first maximal logit, a NaN counting as the maximum (np.argmax); needs C <= 256;
 *   sem8 [V,P,3] = palette[label], palette [palette_entries,3] u8 RGB on the device, palette_entries >= C.
 * bgr != 0 stores rgb8 and sem8 channel-reversed (what cv2.imwrite takes), 0 stores RGB.  sem and palette may be NULL only when sem8 and
 * labels both are.  Argument errors (sizes <= 0, a null plane whose output is asked for, palette_entries < C, labels with C > 256,
 * depth_div == 0 or a non-finite depth parameter, more than 65535 views) return MNF_ERR_INVALID before any HIP call; C > 10239 returns
 * MNF_ERR_UNSUPPORTED; n_views == 0 returns MNF_OK.  Profile label: "frames_views".  Enqueues on `stream` and does not synchronise. */
int mnf_frames_views(const float *rgb, const float *depth, const float *acc, const float *sem,
                     int32_t n_views, int64_t n_pix, int32_t n_classes,
                     const uint8_t *palette, int32_t palette_entries,
                     double depth_mul, double depth_div, double depth_clip_hi, double depth_gain,
                     int32_t bgr,
                     uint8_t *rgb8, uint8_t *dep8, uint8_t *occ8, uint8_t *sem8, uint8_t *labels,
                     mnf_stream_t stream);

/* ---------------------------------------------------------------- semantic object map */

/* The object count of scripts/eval/eval_pipeline_offline.py ("objects detected over planning steps"): one voxel grid per class filled
 * from depth and label images, its clusters, and their greedy match to the ground-truth object positions.
 *
 * The map is a caller-owned, persistent bit grid uint32 bits[C][wpp] over res_x x res_y x res_z voxels of edge voxel_size whose corner
 * is grid_min (three host floats): voxel (x, y, z) of class c is bit (lin & 31) of word c * wpp + (lin >> 5) with
 * lin = (x * res_y + y) * res_z + z (the estimator's layout) and wpp = ceil(X Y Z / 32) ROUNDED UP TO AN EVEN NUMBER, so that every
 * plane starts 8-byte aligned (at most 32 + 31 padding bits per plane; they are never set and every reader masks them).
 * mnf_object_map_bytes returns C * wpp * 4, or 0 for a geometry the map does not index (a non-positive size, an axis above 2^24,
 * more than 2^31 - 64 voxels per class or 2^31 - 1 words in all).  Clearing the map is a memset to 0.
 *
 * mnf_object_map_insert replaces eval_pipeline_offline.py:119-138 (per view and class: the depth image with every other class set to
 * NaN, through VoxelGrid.insert_depth_image; VoxelGrid itself is not part of the reference tree, so the voxelisation is defined here).
 * It ORs n_rays pixels into the map: origins, viewdirs [N,3] f32 (what mnf_generate_rays writes), depth [N] f32 (the distance along
 * the ray), acc [N] f32 or NULL, and exactly one label source: sem [N,C] f32 logits, whose class is the first maximal logit (the label
 * mnf_eval_views predicts), or labels [N], int64 or, with label_is_u8, uint8.  A pixel is skipped when its class is < first_class or
 * >= C (the reference skips label 0: first_class = 1), when its depth is NaN or infinite, <= min_depth or > max_depth, or when acc is
 * given and acc < min_acc.  Otherwise, per axis in float32, each operation rounded separately: p = o + depth * d,
 * i = floor((p - grid_min) * inv) with inv = 1.0f / voxel_size; the pixel is kept when 0 <= i < res on all three axes and sets its
 * voxel's bit (a plain load first, a 32-bit atomic OR only where the bit is clear).  Inserts accumulate.  n_rays == 0 returns MNF_OK.
 *
 * mnf_object_map_count writes the set voxels per class (popcount) to counts [C] int64 on the device.
 *
 * mnf_object_map_clusters replaces eval_pipeline_offline.py:26-42 (get_pointcloud, DBSCAN(eps=0.2, min_samples=1), np.mean per
 * label).  Two voxels of one class are linked when their INTEGER offset has dx^2 + dy^2 + dz^2 <= link_r2 (1 .. 8; 4 is the
 * reference's radius of two voxels, 3 the 26-neighbourhood); the clusters are the connected components, which is DBSCAN(eps =
 * sqrt(link_r2), min_samples = 1) on the integer coordinates.  (On the float centres (i + 0.5) * 0.1 the distance of two voxels two
 * apart comes out as 0.2 or as 0.20000000000000004 depending on i, and eps = 0.2 links only some of them.)  Clusters of fewer than
 * min_cluster_voxels (>= 1) voxels are dropped.  Clusters are ordered by class, then by the smallest linear index they hold.
 * Outputs on the device: clusters [max_clusters,5] f64 rows (class, voxel count, cx, cy, cz) with
 * c = (double)grid_min + (sum / count + 0.5) * (double)voxel_size from exact int64 coordinate sums; cluster_counts [C] int64, the
 * kept clusters per class; info [4] int64 = {set voxels, kept clusters, set voxels > max_voxels, kept clusters > max_clusters}; and,
 * when non-NULL, the labelled point cloud: voxel_ids [max_voxels] int64 = class * (X Y Z) + lin in ascending order and voxel_cluster
 * [max_voxels] int32, the row number of each voxel's cluster (its true number, also where that is >= max_clusters) or -1 where the
 * cluster was dropped.  When the set voxels exceed max_voxels only info is written; when the kept clusters exceed max_clusters the
 * first max_clusters rows are written and info[1] and cluster_counts hold the true numbers.  Nothing is written past a capacity.
 * All sums are integer: the same map gives the same bytes.  workspace: mnf_object_map_clusters_workspace_bytes(C, X, Y, Z,
 * max_voxels) bytes (0 for bad arguments), 8-byte aligned.
 *
 * mnf_object_map_match replaces eval_pipeline_offline.py:45-70.  gt_locs [G,3] f64 and gt_class [G] int32 on the device are the
 * ground-truth objects, in index order within a class.  Per class the clusters are walked in row order: each takes the nearest
 * still-unmatched object of its class, distance sqrt((dx dx + dy dy) + dz dz) in float64, provided that distance is strictly below
 * det_dist_thresh and strictly below 10.0; of equal distances the lowest index wins; a matched object is out of the running.
 * Outputs: detected [C] int32 (what update_sem_step returns), match [max_clusters] int32 = the object of each written row or -1 (rows
 * that clusters did not write are not touched), gt_match [G] int32 = the row that took each object or -1.  `clusters` and `info` are
 * mnf_object_map_clusters' outputs, max_clusters the capacity they were written with.
 *
 * Argument errors (a null required pointer, a non-positive resolution or voxel_size, link_r2 outside 1 .. 8, both label sources or
 * neither, first_class outside [0, C), a negative capacity, a misaligned workspace or one that is too small) return MNF_ERR_INVALID
 * before any HIP call.  Profile labels: "object_map_insert", "object_map_count", "object_map_clusters", "object_map_match".  Every
 * call enqueues on `stream` and none synchronises. */
int64_t mnf_object_map_bytes(int32_t n_classes, int32_t res_x, int32_t res_y, int32_t res_z);
int mnf_object_map_insert(uint32_t *bits, int32_t n_classes, int32_t res_x, int32_t res_y, int32_t res_z, const float *grid_min_host,
                          float voxel_size, int32_t first_class, const float *origins, const float *viewdirs, const float *depth,
                          const float *acc, const float *sem, const void *labels, int32_t label_is_u8, int64_t n_rays,
                          float min_depth, float max_depth, float min_acc, mnf_stream_t stream);
int mnf_object_map_count(const uint32_t *bits, int32_t n_classes, int32_t res_x, int32_t res_y, int32_t res_z, int64_t *counts,
                         mnf_stream_t stream);
int64_t mnf_object_map_clusters_workspace_bytes(int32_t n_classes, int32_t res_x, int32_t res_y, int32_t res_z, int64_t max_voxels);
int mnf_object_map_clusters(const uint32_t *bits, int32_t n_classes, int32_t res_x, int32_t res_y, int32_t res_z,
                            const float *grid_min_host, float voxel_size, int32_t link_r2, int32_t min_cluster_voxels,
                            int64_t max_voxels, int64_t max_clusters, double *clusters, int64_t *cluster_counts, int64_t *info,
                            int64_t *voxel_ids, int32_t *voxel_cluster, void *workspace, int64_t workspace_bytes, mnf_stream_t stream);
int mnf_object_map_match(const double *clusters, const int64_t *info, int64_t max_clusters, int32_t n_classes, const double *gt_locs,
                         const int32_t *gt_class, int32_t n_gt, double det_dist_thresh, int32_t *detected, int32_t *match,
                         int32_t *gt_match, mnf_stream_t stream);

/* ---------------------------------------------------------------- exploration map */

/* The occupancy side of scripts/eval/frontier_baseline.py, the paper's comparison policy: every pixel of a depth image is ray-cast
 * through a voxel grid (:170), the top-down view of the grid (:188) gives frontier cells (:52-67), those are clustered and the member
 * nearest to the current pose of each cluster is a goal (:191-214).  The same map gives explored volume per planning step.
 *
 * The map is a caller-owned, persistent bit grid uint32 bits[2][wpp]: plane 0 is "a ray passed through", plane 1 is "a ray ended
 * here".  Voxel indexing (lin = (x * res_y + y) * res_z + z, bit (lin & 31) of word plane * wpp + (lin >> 5)), wpp rounded up to an
 * even number, the tail bits (never set, masked by every reader) and the limits on the geometry are the semantic object map's, above.
 * mnf_explore_map_bytes returns 2 * wpp * 4, or 0 for a geometry that is refused.  Clearing the map is a memset to 0.  A voxel reads
 * as OCCUPIED if its plane-1 bit is set, else FREE if its plane-0 bit is set, else UNKNOWN.
 *
 * mnf_explore_map_insert (VoxelGrid is not part of the reference tree, so the ray-cast is defined here).  origins, viewdirs [N,3] f32,
 * depth [N] f32 (the distance along the ray), acc [N] f32 or NULL.  One launch, no host synchronisation; n_rays == 0 returns MNF_OK.
 * Per pixel, in float32, each operation rounded separately (g = grid_min, three host floats; inv = 1.0f / voxel_size):
 *   1. The pixel is skipped when depth is NaN, when depth <= min_depth (Habitat writes 0 for no data), when acc is given and
 *      acc < min_acc, or when a component of o or d is not finite.
 *   2. hit = depth is finite && depth <= max_range; t = hit ? depth : max_range.  (+inf, or a depth beyond the range, carves free space
 *      out to max_range and marks nothing occupied.)
 *   3. Per axis k: a_k = floor((o_k - g_k) * inv), p_k = o_k + t * d_k, b_k = floor((p_k - g_k) * inv).  The pixel is skipped when
 *      some |a_k| or |b_k| is >= 2^24.  n_k = |b_k - a_k|, s_k = sign(b_k - a_k).
 *   4. For the axes with n_k > 0 (so d_k != 0): edge_k = (float)(a_k + (s_k > 0 ? 1 : 0)) * voxel_size,
 *      tm_k = ((g_k + edge_k) - o_k) / d_k, td_k = voxel_size / |d_k|.
 *   5. The walk takes exactly n_x + n_y + n_z steps from voxel a.  Each step: the candidate is the first axis in x, y, z order with
 *      n_k > 0; a later axis with n_k > 0 replaces it only if its tm is STRICTLY smaller.  The chosen axis moves by s_k, n_k -= 1,
 *      tm_k = tm_k + td_k.  The walk therefore ends in voxel b whatever the rounding.
 *   6. Every visited voxel but the last gets the free bit; the last, b, gets the occupied bit if hit, else the free bit.  Only voxels
 *      inside the grid are written (a plain load first, a 32-bit atomic OR only where a bit is clear); voxels outside are walked or,
 *      once the ray has left the box for good, skipped.  Only the resulting bits are specified.
 * Inserts accumulate, and the bits do not depend on the order or the grouping of the pixels.  stats, when non-NULL, is int64 [2] on the
 * device to which the call ADDS {voxel steps walked, atomic ORs issued} (a measurement aid; the second depends on the schedule).
 * With the same grid, max_depth = max_range and labels all >= first_class, plane 1 equals the OR over the classes of a semantic object
 * map given the same pixels.
 *
 * Read-outs (device outputs, integer sums):
 * mnf_explore_map_count writes counts [3] int64 = {free, occupied, unknown} voxels.
 * mnf_explore_map_topdown writes map [X][Z] int8 over the layers y_lo <= y < y_hi (0 <= y_lo <= y_hi <= res_y): 1 if a voxel of the
 * column slab is occupied, else 0 if one is free, else -1: the grid frontier_baseline.py:188 reads.
 * mnf_explore_map_frontiers replaces find_frontiers on such a map [X][Z] (any int8 map of -1 / 0 / 1).  A cell of value 0 is a
 * frontier cell when an in-bounds cell of its 3 x 3 neighbourhood is -1.  The reference's `break` leaves only the inner loop, so it
 * appends a cell once per dx in {-1, 0, 1} whose column x + dx holds an unknown neighbour: each frontier cell carries that
 * MULTIPLICITY, 1 .. 3.  cells [max_frontiers,2] int32 (x, z) in ascending x * Z + z, mult [max_frontiers] int32, info [2] int64 =
 * {frontier cells, frontier cells > max_frontiers}; the first max_frontiers are written, nothing past the capacity.
 * mnf_explore_map_frontier_clusters replaces DBSCAN(eps=1, min_samples=3) and the nearest member per cluster on the first
 * min(frontier_info[0], max_frontiers) cells of such a list (frontier_info is read on the device: no host copy in between).  Two
 * cells are linked when their INTEGER offset has dx^2 + dz^2 <= eps2 (1 .. 8); a cell's neighbourhood is itself plus the cells linked
 * to it; a cell is CORE when the multiplicities of its neighbourhood sum to >= min_samples (weighted == 0: every multiplicity counts
 * 1); the clusters are the connected components of the core cells, numbered by their smallest row-major core cell; a non-core cell
 * with a core neighbour takes the SMALLEST label among those neighbours; every other cell is -1.  This is what scikit-learn's DBSCAN
 * gives on the duplicated list, and with sample_weight = mult, numbering included.  The goal of a cluster is its member cell (core or
 * not) with the smallest dx * dx + dz * dz, dx = (double)x - current_x, dz = (double)z - current_z in float64 in that order; of
 * equal distances the lowest row-major cell wins.  labels [max_frontiers] int32 (the true number, also where it is >=
 * max_clusters), goals [max_clusters,2] int32 and sizes [max_clusters] int32 (member cells; 0 beyond the clusters found), info [2]
 * int64 = {clusters, clusters > max_clusters}.  workspace: mnf_explore_map_frontier_clusters_workspace_bytes(X, Z, max_frontiers,
 * max_clusters) bytes (0 for bad arguments), 8-byte aligned.
 *
 * Argument errors (a null required pointer, a non-positive resolution or voxel_size, max_range not finite or <= 0,
 * max_range / voxel_size > 2^20, layers outside the grid, eps2 outside 1 .. 8, min_samples < 1, a negative capacity, a current that is
 * not finite, a misaligned workspace or one that is too small) return MNF_ERR_INVALID before any HIP call.  Profile labels:
 * "explore_map_insert", "explore_map_count", "explore_map_topdown", "explore_map_frontiers", "explore_map_frontier_clusters".  Every
 * call enqueues on `stream` and none synchronises. */
int64_t mnf_explore_map_bytes(int32_t res_x, int32_t res_y, int32_t res_z);
int mnf_explore_map_insert(uint32_t *bits, int32_t res_x, int32_t res_y, int32_t res_z, const float *grid_min_host, float voxel_size,
                           float max_range, const float *origins, const float *viewdirs, const float *depth, const float *acc,
                           int64_t n_rays, float min_depth, float min_acc, int64_t *stats, mnf_stream_t stream);
int mnf_explore_map_count(const uint32_t *bits, int32_t res_x, int32_t res_y, int32_t res_z, int64_t *counts, mnf_stream_t stream);
int mnf_explore_map_topdown(const uint32_t *bits, int32_t res_x, int32_t res_y, int32_t res_z, int32_t y_lo, int32_t y_hi, int8_t *map,
                            mnf_stream_t stream);
int mnf_explore_map_frontiers(const int8_t *map, int32_t res_x, int32_t res_z, int64_t max_frontiers, int32_t *cells, int32_t *mult,
                              int64_t *info, mnf_stream_t stream);
int64_t mnf_explore_map_frontier_clusters_workspace_bytes(int32_t res_x, int32_t res_z, int64_t max_frontiers, int64_t max_clusters);
int mnf_explore_map_frontier_clusters(const int32_t *cells, const int32_t *mult, const int64_t *frontier_info, int64_t max_frontiers,
                                      int32_t res_x, int32_t res_z, int32_t eps2, int32_t min_samples, int32_t weighted,
                                      double current_x, double current_z, int64_t max_clusters, int32_t *labels, int32_t *goals,
                                      int32_t *sizes, int64_t *info, void *workspace, int64_t workspace_bytes, mnf_stream_t stream);

/* ---------------------------------------------------------------- planner grid search */

/* The first step of the planner, Dijkstra(aabb, path_finding_map, voxel_grid_size, 0.05).planning(...) of planning/dijkstra.py:72-182, which
 * sample_traj calls once per sampled goal (planning/planning_funcs.py:288-326), as a single-source shortest-path FIELD over the map and
 * paths read back out of it: one field per start cell answers every goal from that start: reached or not, at what cost, along which cells.
 *
 * The grid and the moves.  A map is blocked [nx][ny] int32, non-zero = obstacle, indexed [x][y] as verify_node indexes
 * obstacle_map[node.x][node.y] (dijkstra.py:194-215): mnf_planner_map's output as it stands.  A move goes to one of the 8 neighbours,
 * straight cost 1, diagonal cost sqrt(2) (dijkstra.py:247-260).  A move is legal when the cell moved TO lies in [0, lim_x) x [0, lim_y)
 * and is not blocked; nothing else is checked: a diagonal move between two obstacles that touch at a corner is legal, as in the
 * reference.  The source has cost 0 whether or not it is blocked or within the limits: the reference never verifies its start node.
 * lim_x <= nx and lim_y <= ny stand for the reference's `px >= self.max_x` / `py >= self.max_y` tests.
 *
 * Costs are exact integers, not accumulated floats.  A way of a straight and b diagonal moves costs a + b sqrt(2); two different pairs
 * never cost the same (sqrt(2) is irrational), so the cheapest (a, b) of a cell is unique.  A cell's LABEL is the uint32 (a << 16) | b;
 * 0xFFFFFFFF = not reached: blocked cells, cells beyond the limits, cells cut off, and the whole field of a source outside
 * [0, nx) x [0, ny).  Labels are ordered by the exact sign of da + db sqrt(2): where the signs of da and db agree, that sign; otherwise
 * da^2 against 2 db^2 in integers.  (A float64 a + b sqrt(2) formed freshly from the two integers orders them the same way: its rounding
 * error is below 2^-36 for a, b < 2^16 and distinct costs are more than 2^-18 apart.)  No cost is built by adding move after move.
 *
 * Size cap: (nx + 2)(ny + 2) <= 40 000, so that a field with a one-cell border, 160 000 B, fits the LDS of one CU and
 * a + b <= nx ny - 1 < 2^16: up to 198 x 198.  Larger maps are refused; there is no second route through global memory.
 *
 * mnf_path_field_bytes returns nx * ny * n_sources * 4, the bytes of `field`, or 0 for a geometry that is refused or n_sources < 0.
 * mnf_path_field: blocked [n_maps][nx][ny] with n_maps == 1 (one map for every source) or n_maps == n_sources (a map per source); sources
 * [n_sources][2] int32 (x, y) on the device; field [n_sources][nx][ny] uint32; info [n_sources][2] int64 = {reached cells (the source
 * included), sweeps run}.  One workgroup per source relaxes the labels in LDS, sweep after sweep, until a sweep changes nothing; the
 * fixpoint is unique, so the field does not depend on the schedule.  A fixpoint needs at most nx ny sweeps; the kernel stops after that
 * many whatever happens and then writes info[b][0] = -1 (a logic error: the field of that source is not to be used).  n_sources == 0 is a
 * legal no-op.
 *
 * The path of a goal is fixed by the field alone (no parent array, no race).  From a reached cell c with label (a, b) step to c - m for
 * the FIRST move m in the reference's motion order (1,0), (0,1), (-1,0), (0,-1), (-1,-1), (-1,1), (1,-1), (1,1) for which c - m lies
 * inside the map and carries exactly the label (a - 1, b) for a straight m, (a, b - 1) for a diagonal m; repeat until label 0.  The path
 * lists the cells goal first, source last, a + b + 1 of them, as calc_final_path lists them (dijkstra.py:170-182).  It is A shortest
 * path, of the reference's cost and make-up; of several equal ones the reference returns the one the insertion order of its Python dict
 * leads to, which need not be this one.
 * mnf_path_trace: field [n_fields][nx][ny]; goals [n_goals][3] int32 = {field index, x, y}; offsets [n_goals + 1] int64 into paths
 * [total][2] int32 (x, y), which the caller sizes; info [2] int64 = {goals whose path was written, goals whose slot did not fit}.  One
 * lane per goal.  The length of a goal is a + b + 1, or 0 when it is not reached, lies outside the map or names no field.  A goal whose
 * slot offsets[g + 1] - offsets[g] differs from its length gets nothing written and counts in info[1]; a goal of length 0 that fits
 * counts in neither.
 *
 * Argument errors (a null required pointer, a size that is not positive or beyond the cap, limits outside [0, nx] x [0, ny], n_maps
 * other than 1 or n_sources, a negative count, a misaligned info or offsets) return MNF_ERR_INVALID before any HIP call.  Profile
 * labels: "path_field", "path_trace".  Both calls enqueue on `stream` and neither synchronises. */
int64_t mnf_path_field_bytes(int32_t nx, int32_t ny, int32_t n_sources);
int mnf_path_field(const int32_t *blocked, int32_t n_maps, int32_t nx, int32_t ny, int32_t lim_x, int32_t lim_y, const int32_t *sources,
                   int32_t n_sources, uint32_t *field, int64_t *info, mnf_stream_t stream);
int mnf_path_trace(const uint32_t *field, int32_t n_fields, int32_t nx, int32_t ny, const int32_t *goals, const int64_t *offsets,
                   int64_t n_goals, int32_t *paths, int64_t *info, mnf_stream_t stream);

/* ---------------------------------------------------------------- planner cost map */

/* The planner's 2-D cost map and visit counts, which the reference updates from the middle row of every sampled depth image
 * (update_cost_map, planning/planning_funcs.py:192-219, over generate_ray_casting_grid_map and bresenham,
 * perception/data_proc/depth_to_grid.py:31-73, :142-182; called at scripts/pipeline.py:272-292, :1115-1138 and :1171-1189), and the goal
 * draw of sample_traj: its vm map (planning_funcs.py:262-276) and its draw-and-reject loop (planning_funcs.py:296-326).
 *
 * The scan.  depth [n_views][height][width] f32; the kernel reads row height / 2 of every view as a planar scan of `width` beams.  align
 * [width] f64 (the angle of a column from the optical axis), yaw [n_views] f64, loc [n_views][2] f64 (world x and z of the camera), centre
 * [n_views][2] int32 (the camera's cell, g_loc[0] and g_loc[2] of the reference), all on the device; aabb_host six host doubles, res the
 * cell size; the grid is nx x nz cells.  Per view in order and per beam j in order, in float64 with every operation rounded on its own
 * (d = the depth widened to float64):
 *   a  = (align[j] + yaw) mod 2 pi, with Python's sign rule (fmod, plus 2 pi where that is negative);
 *   ox = sin(-a) d + loc_x,   oy = (-cos(-a)) d + loc_z;
 *   ix = rint((ox - aabb[2]) / res),   iy = rint((oy - aabb[0]) / res)   (round-half-even, Python's round).
 * The reference subtracts aabb[2] from an x coordinate and aabb[0] from a z coordinate; that is reproduced, not repaired.
 * Every cell of the reference's Bresenham walk from centre to (ix, iy) becomes FREE.  The walk (depth_to_grid.py:31-73): with (x1, y1) =
 * centre and (x2, y2) = (ix, iy), swap x and y of both ends when |y2 - y1| > |x2 - x1| ("steep"), then swap the ends when x1 > x2; with
 * dx = x2 - x1, e0 = dx / 2 (integer) and ystep = 1 if y1 < y2 else -1, column k = 0 .. dx holds the cell (x1 + k, y1 + ystep s_k) (swapped
 * back when steep), where s_k = 0 for dx = 0 and otherwise (k |y2 - y1| - e0 + dx - 1) / dx in integer division: the number of times the
 * loop's error term has gone negative before column k.  Then the cells (ix, iy), (ix + 1, iy), (ix, iy + 1), (ix + 1, iy + 1) become
 * OCCUPIED.  A later write wins, within a view and across views.  After a view, cost is 1.0 where the view left a cell occupied, 0.0 where
 * it left it free, and a cell it left free adds one to that cell's visit count (visiting_map, which the callers sum over views).
 * Order without a serial loop: every write carries the key 2 j + occ + 1; keys are combined with an integer max on the view's plane, a cell's
 * state in a view is (largest key - 1) & 1, and views are ordered the same way by the key 2 (v + 1) + occ.  All atomics are integer max
 * or add; the result does not depend on the schedule and no floating-point value is accumulated.
 * Cells outside the grid.  A cell at or beyond the grid on the high side is skipped, as in the reference.  A cell with a NEGATIVE index is
 * skipped too and its beam counted: the reference wraps such a cell round through Python's negative indexing, or raises.  This is the one
 * deliberate difference.  A beam whose depth is not finite is skipped whole and counted; so is a beam whose end cell or centre lies
 * beyond +-2^30 in either index (a NaN among yaw, loc or align ends here too).  The work of a beam is bounded by the grid, not by its depth.
 *
 * State: mnf_scan_map_bytes(nx, nz) = 3 * nx * nz * 4 bytes, or 0 for a grid outside the planner's cap (nx + 2)(nz + 2) <= 40 000: three
 * int32 planes [nx][nz], the cost code (0 unknown = 0.5, 1 free = 0.0, 2 occupied = 1.0), the visit counts, and a scratch plane the update
 * clears itself.  A new map is a memset to 0.  mnf_scan_map_update adds to info [4] int64 = {beams with a negative cell, beams with a
 * non-finite depth, beams beyond +-2^30, beams drawn (the first kind included)}; the caller clears it.  One launch walks every view of the
 * batch (one workgroup per view, its key plane in LDS), a second small one writes the cost codes.  n_views == 0 is a legal no-op.  A batch
 * and the same views given one call at a time leave the same cost codes, visit counts and info.
 *
 * mnf_planner_goal_map.  blocked [nx][nz] int32 (mnf_planner_map's output as it stands; a cell is FREE when its value is not above 0, the
 * reference's `> 1e-4` on integers), visits [nx][nz] int32, field [nx][nz] uint32 of mnf_path_field for the start cell, or NULL.
 *   vm [nx][nz] f64 = -1 on blocked cells, decay[visits - least] on free ones, least = the smallest visit count of a free cell; decay
 *   [n_decay] f64 is the caller's table decay[m] = exp(-m / 5) in float64 (a difference of n_decay or more reads as 0.0, which
 *   exp(-m / 5) is from m = 3727 on), so vm holds the bytes the caller's own exp gives, as planning_funcs.py:268-276 forms them.
 *   cells [nx nz][2] int32: the cells with vm >= 0 that, where a field is given, are reached in it, in row-major order (np.argwhere's), by an
 *   ordered prefix sum; rows from count on are -1.  count [1] int64.  The same inputs give the same bytes.
 * mnf_planner_goal_pick.  u [n_draws] f64 in [0, 1) from the caller's generator; goals [n_draws][2] int32 = cells[min(floor(u n), n - 1)]
 * with n = min(count[0], max_cells) read on the device, (-1, -1) when n is 0; a u below 0 or NaN takes the first cell.  This has the
 * distribution of the reference's loop (a uniform free cell, redrawn until planning() finds a way); it does not reproduce the
 * reference's random stream.  The reference's visit weighting is multiplied by 0 (planning_funcs.py:301) and is left out.
 *
 * Argument errors (a null required pointer, a size that is not positive or beyond the cap, a height or width that is not positive, a
 * negative count, an aabb or res that is not finite, res <= 0, n_decay < 1, a misaligned pointer) return MNF_ERR_INVALID before any
 * HIP call.  Profile labels: "scan_map_update", "planner_goal_map", "planner_goal_pick".  Every call enqueues on `stream` and none
 * synchronises.  There is no CPU fallback. */
int64_t mnf_scan_map_bytes(int32_t nx, int32_t nz);
int mnf_scan_map_update(void *state, int32_t nx, int32_t nz, const float *depth, int32_t n_views, int32_t height, int32_t width,
                        const double *align, const double *yaw, const double *loc, const int32_t *centre, const double *aabb_host, double res,
                        int64_t *info, mnf_stream_t stream);
int mnf_planner_goal_map(const int32_t *blocked, const int32_t *visits, const uint32_t *field, int32_t nx, int32_t nz, const double *decay,
                         int32_t n_decay, double *vm, int32_t *cells, int64_t *count, mnf_stream_t stream);
int mnf_planner_goal_pick(const int32_t *cells, const int64_t *count, int64_t max_cells, const double *u, int64_t n_draws, int32_t *goals,
                          mnf_stream_t stream);

/* ---------------------------------------------------------------- surface mesh */

/* The geometry a trained field has learnt as a triangle mesh with colours and classes: what the `extract_mesh` of the reference's nerfacc
 * benchmarks does with a host package, and what simulator/build_point_cloud_from_mesh.py's semantic ground-truth cloud is compared with.
 * Three parts: the iso-surface of ANY scalar lattice (1), the lattice of a trained field (2), the attributes of the vertices (3).
 *
 * 1. mnf_surface_extract: marching tetrahedra on the Kuhn split.
 * Input: values [X+1][Y+1][Z+1] f32 on the device, x slowest, X = cells_x etc. (1 .. 1024 each); lin(p) = (x (Y+1) + y)(Z+1) + z.  A lattice
 * point is INSIDE when value > iso: NaN is outside, and so is a value equal to iso.
 * Tetrahedra.  Every cell c is cut into the same six tetrahedra around its main diagonal; tetrahedron k belongs to the k-th axis
 * permutation pi in the order (x,y,z), (x,z,y), (y,x,z), (y,z,x), (z,x,y), (z,y,x) and has the vertices v0 = c, v1 = v0 + e_pi1,
 * v2 = v1 + e_pi2, v3 = c + (1,1,1).  Neighbouring cells cut their common face the same way, so the mesh is watertight and manifold.
 * Edges.  Every tetrahedron edge has one of 7 directions d, its TYPE: 0 (1,0,0), 1 (0,1,0), 2 (0,0,1), 3 (1,1,0), 4 (1,0,1), 5 (0,1,1),
 * 6 (1,1,1), and is owned by its lower end p (the other end is p + d).  An edge whose ends differ in inside-ness carries exactly one vertex.
 * Vertices, in ascending (lin(p), type).  In float32, every operation rounded on its own (a = values[p], b = values[p + d]):
 *   t = (iso - a) / (b - a), or 0.5f when a or b is not finite;
 *   pos_k = ((float)p_k + t * (float)d_k) * step_k + origin_k.
 * Normals.  The lattice difference of axis k at a point q with coordinate i of n points: (values[q + e_k] - values[q - e_k]) * 0.5f for
 * 0 < i < n - 1, values[q + e_k] - values[q] for i = 0, values[q] - values[q - e_k] for i = n - 1; a difference that is not finite counts
 * as 0.  With ga, gb those of p and p + d:  g_k = ga_k + t * (gb_k - ga_k);  m_k = (-g_k) / step_k;
 * len = sqrtf((m_x m_x + m_y m_y) + m_z m_z);  normal_k = m_k / len, or (0,0,0) when len is 0 or not finite.  (The normal points out of
 * the matter: down the gradient.)
 * Triangles, in ascending (cell (x Y + y) Z + z, tetrahedron, triangle).  With the tetrahedron's vertices numbered 0..3 and "ab" the
 * vertex on the edge between a and b:
 *   one inside a, outside b < c < d:        (ab, ac, ad)
 *   three inside a < b < c, outside d:      (ad, bd, cd)
 *   two inside a < b, outside c < d:        (ac, ad, bd), then (ac, bd, bc)
 * The last two indices of a triangle are swapped where needed so that (q1 - q0) x (q2 - q0) points from the mean of the tetrahedron's inside
 * vertices to the mean of its outside vertices, evaluated with every crossing at the midpoint of its edge; the sign does not depend on t,
 * so the swap is a constant of (k, inside bits).
 * Outputs: positions, normals [max_vertices,3] f32, triangles [max_triangles,3] int32 (vertex indices), info [4] int64 = {vertices,
 * triangles, vertices - max_vertices if positive else 0, triangles - max_triangles if positive else 0}.  Vertex r is written iff
 * r < max_vertices; triangle r iff r < max_triangles and its three indices are < max_vertices (it is counted either way, and its slot is
 * then left as it was).  Nothing is written past either capacity; capacities of 0 (outputs may be NULL) make a counting call.
 * The mesh is OPEN where matter touches the lattice boundary: no triangle is made on the boundary faces themselves.
 * workspace: mnf_surface_extract_workspace_bytes(X, Y, Z) bytes (0 for a refused size; about 4.1 bytes per lattice point), 8-byte aligned.
 *
 * mnf_surface_measure: out [2] float64 = {area, enclosed volume} of the first min(info[1], max_triangles) triangles, info read on the
 * device.  Each triangle (a, b, c), its positions widened to float64, adds |(b - a) x (c - a)| / 2 and a . (b x c) / 6; the order of the
 * sum is not specified.  A triangle with an index outside [0, min(info[0], max_vertices)) adds nothing.  Meaningful when info[2] == info[3] == 0.
 *
 * 2. mnf_surface_lattice_points.  binaries [RX][RY][RZ] uint8 (level 0 of the estimator, non-zero = occupied), refine in {1, 2, 4, 8}, aabb
 * six host floats.  The lattice has (R_k refine + 1) points per axis (R_k refine <= 1024); point i of an axis touches the cells
 * (i - 1) / refine and i / refine (integer division) that exist: two where i is a multiple of refine, else one.  A point is LISTED when a
 * cell it touches is occupied or has an occupied cell in its 3 x 3 x 3 neighbourhood clipped at the grid.  The list is in ascending lin:
 * lin [max_points] int32, positions [max_points,3] f32 with pos_k = aabb_k + (float)i_k * step_k, step_k = (aabb_{3+k} - aabb_k) /
 * (float)(R_k refine), in float32; info [2] int64 = {points, points - max_points if positive else 0}; nothing is written past the
 * capacity.  (origin = aabb_0..2 and this step are what mnf_surface_extract takes for such a lattice.)
 * mnf_surface_lattice_scatter fills values [n_values] with 0 and then writes values[lin[i]] = density[i] for i < min(point_info[0],
 * max_points), point_info read on the device (a lin outside [0, n_values) is skipped).  Densities are never negative, so with iso > 0 no
 * surface appears where nothing was evaluated.  The densities come from mnf_field_density at the listed positions.
 *
 * 3. mnf_surface_vertex_attrs.  rgb [n,3], sem [n,C] f32 as mnf_field_forward writes them; palette [C,3] uint8 (further rows are not read) or NULL.
 *   colour [n,3] uint8 = (uint8)(min(max(c, 0), 1) * 255.0f + 0.5f) in float32, 0 for NaN;
 *   label [n] int32 = the first index of the largest logit, -1 when a logit of the row is NaN;
 *   sem_colour [n,3] uint8 = palette[label], (0,0,0) for label -1.
 * Any output may be NULL; sem_colour needs the palette.
 *
 * Argument errors (a null required pointer, a size outside the limits, a step that is not finite or not positive, an iso that is not finite,
 * a refine other than 1, 2, 4, 8, an aabb that is empty or not finite, a negative capacity or one >= 2^31, a workspace or info that is
 * misaligned, a workspace that is too small) return MNF_ERR_INVALID before any HIP call.  Profile labels: "surface_extract",
 * "surface_measure", "surface_lattice_points", "surface_lattice_scatter", "surface_vertex_attrs".  Every call enqueues on `stream` and
 * none synchronises. */
int64_t mnf_surface_extract_workspace_bytes(int32_t cells_x, int32_t cells_y, int32_t cells_z);
int mnf_surface_extract(const float *values, int32_t cells_x, int32_t cells_y, int32_t cells_z, float iso, const float *origin_host,
                        const float *step_host, int64_t max_vertices, int64_t max_triangles, float *positions, float *normals,
                        int32_t *triangles, int64_t *info, void *workspace, int64_t workspace_bytes, mnf_stream_t stream);
int mnf_surface_measure(const float *positions, const int32_t *triangles, const int64_t *info, int64_t max_vertices, int64_t max_triangles,
                        double *out, mnf_stream_t stream);
int64_t mnf_surface_lattice_points_workspace_bytes(int32_t res_x, int32_t res_y, int32_t res_z, int32_t refine);
int mnf_surface_lattice_points(const uint8_t *binaries, int32_t res_x, int32_t res_y, int32_t res_z, int32_t refine, const float *aabb_host,
                               int64_t max_points, int32_t *lin, float *positions, int64_t *info, void *workspace, int64_t workspace_bytes,
                               mnf_stream_t stream);
int mnf_surface_lattice_scatter(const float *density, const int32_t *lin, const int64_t *point_info, int64_t max_points, float *values,
                                int64_t n_values, mnf_stream_t stream);
int mnf_surface_vertex_attrs(const float *rgb, const float *sem, int64_t n, int32_t n_classes, const uint8_t *palette, uint8_t *colour,
                             int32_t *label, uint8_t *sem_colour, mnf_stream_t stream);

/* ---------------------------------------------------------------- mesh quality */

/* How good the map is as geometry: the surface mesh above against a ground-truth cloud such as simulator/build_point_cloud_from_mesh.py
 * writes.  Three parts: points sampled on triangles (1), the nearest neighbour of every point of one cloud in another within a radius (2), the
 * reduction of the distances to what accuracy, completion, precision, recall and a class confusion matrix are made of (3).
 *
 * 1. mnf_cloud_sample_triangles: the sampling of build_point_cloud_from_mesh.py:47-83.
 * Input: positions [V,3] f32, triangles [T,3] int32 (V, T < 2^31), res > 0 (float64).  Per triangle (p1, p2, p3), widened to float64, every
 * operation rounded on its own, |e| = sqrt((e_x e_x + e_y e_y) + e_z e_z):
 *   the three vertices p1, p2, p3 as they are;
 *   d1 = |p2 - p1|, n1 = (p2 - p1) / d1, d2 = |p3 - p1|, n2 = (p3 - p1) / d2;
 *   for k = 0 .. count(d1 / res) - 1, i = (double)k * res:  b = ((d1 - i) * d2) / d1;
 *     for l = 0 .. count(b / res) - 1, j = (double)l * res:  the point (p1 + i * n1) + j * n2, per component.
 * count(x) = ceil(x) for x > 0, else 0 (numpy's arange), and it saturates at 2^31.  A triangle with d1 == 0, d2 == 0 or a vertex that is not
 * finite gives its three vertices only; a triangle with an index outside [0, V) gives nothing.
 * ROWS.  The work is laid out by row: row 0 of a triangle is its three vertices, row 1 + k the k-th pass of the outer loop; a triangle has 0
 * (bad index), 1 (vertices only) or 1 + count(d1 / res) rows.  The caller gives the row capacity `max_rows` (< 2^31) the workspace is sized for.
 * Outputs, in ascending (triangle, row, l): points [max_points,3] f32 = the double rounded to float32, face [max_points] int32 = the triangle
 * the point came from, info [2] int64 = {points, points - max_points if positive else 0}.  Point r is written iff r < max_points; nothing is
 * written past the capacity; max_points = 0 (points and face may be NULL) makes a counting call.  When the triangles have more rows than
 * max_rows the points cannot be counted: nothing is written and info = {-1, rows}; call again with max_rows >= rows (max_rows = 0 asks for
 * just that).  A mesh in which a count saturates has more than 2^31 - 1 points, which no capacity admits (max_points < 2^31): info[0] is then a
 * lower bound and info[1] > 0.
 * workspace: mnf_cloud_sample_triangles_workspace_bytes(T, max_rows) bytes (0 for a refused size; 16 B per triangle, 20 B per row and the
 * scan's own), 8-byte aligned.
 *
 * 2. mnf_cloud_nearest.  query [n,3], target [m,3] f32 (n, m < 2^31), r_max >= 2^-60 with a finite float32 square (so that r_max * r_max
 * is a normal float32 and no rounding of d2 is worse than relative), box six host floats (min, max).
 * In float32, every operation rounded on its own: d2(q, t) = ((q_x - t_x)^2 + (q_y - t_y)^2) + (q_z - t_z)^2.  Per query:
 *   index [n] int32 = the target with the smallest d2 among those with d2 <= r_max * r_max, the lowest index on a tie; -1 when there is none
 *     or the query has a coordinate that is not finite.  A target with a coordinate that is not finite never matches.
 *   dist [n] f32 = sqrtf(d2) of that target, r_max where index is -1.
 * The result is the brute-force answer over all n m pairs, whatever the box: the box only places the cell list the search uses (cell edge
 * max(r_max (1 + 2^-10), widest box side / 128), at most 128 cells per axis; a point outside the box falls into the border cell next to it).
 * A box that hugs the targets is the fast one.
 * workspace: mnf_cloud_nearest_workspace_bytes(n, m, box, r_max) bytes (0 for refused arguments; 20 B per target, 12 B per query, 32 B per cell
 * and the scan's own), 16-byte aligned.
 *
 * 3. mnf_cloud_distance_stats.  dist, index [n] as (2) wrote them against m targets, query [n,3] or NULL, 0 <= thr <= r_max, and for the confusion
 * matrix query_label [n], target_label [m] int32 and n_classes = C in 1 .. 1024.  A query COUNTS when it is finite (every query when `query` is
 * NULL); it is FOUND when it counts and 0 <= index < m; it is WITHIN when it is found and dist <= thr.
 *   counts [3] int64 = {counting, found, within};
 *   sums [2] float64 = {sum of dist over the counting ones (an unmatched one adds the r_max that (2) wrote), sum of dist over the found ones},
 *     each dist widened to float64; the order of the sums is not specified;
 *   confusion [C,C] int64 or NULL: confusion[a][b] = the WITHIN queries with query_label = a and target_label[index] = b, both in [0, C).
 *
 * Argument errors (a null required pointer, a count outside [0, 2^31), a res, r_max or thr outside its range, a box that is not finite or has
 * max < min, n_classes outside 1 .. 1024, an info, counts, sums, confusion or workspace that is misaligned, a workspace that is too small)
 * return MNF_ERR_INVALID before any HIP call.  Profile labels: "cloud_sample_triangles", "cloud_nearest", "cloud_distance_stats".  Every call
 * enqueues on `stream` and none synchronises. */
int64_t mnf_cloud_sample_triangles_workspace_bytes(int64_t n_triangles, int64_t max_rows);
int mnf_cloud_sample_triangles(const float *positions, int64_t n_vertices, const int32_t *triangles, int64_t n_triangles, double res, int64_t max_rows,
                               int64_t max_points, float *points, int32_t *face, int64_t *info, void *workspace, int64_t workspace_bytes,
                               mnf_stream_t stream);
int64_t mnf_cloud_nearest_workspace_bytes(int64_t n, int64_t m, const float *box_host, float r_max);
int mnf_cloud_nearest(const float *query, int64_t n, const float *target, int64_t m, float r_max, const float *box_host, int32_t *index, float *dist,
                      void *workspace, int64_t workspace_bytes, mnf_stream_t stream);
int mnf_cloud_distance_stats(const float *dist, const int32_t *index, const float *query, int64_t n, float thr, float r_max, const int32_t *query_label,
                             const int32_t *target_label, int64_t m, int32_t n_classes, int64_t *counts, double *sums, int64_t *confusion,
                             mnf_stream_t stream);

/* ---------------------------------------------------------------- trajectory clearance */

/* How far a trajectory stays from what the map calls occupied: the exact squared distance field of the members' occupancy grids (1), samples
 * looked up in it (2), and the reference's voxel walk between two points (3).  Grids are [X][Y][Z], lin = (x Y + y) Z + z, the estimator's
 * layout; 1 <= X, Y, Z <= 2048 and the voxel count within the bit grids' bound (< 2^31 - 64).  LEVEL 0 of the estimator only.
 *
 * 1. mnf_clearance_field.  binaries [n_members][X][Y][Z] uint8 as mnf_planner_map takes them (non-zero = occupied).
 *   d2 [X][Y][Z] int32 = the squared Euclidean distance, in voxels, from each voxel to the nearest voxel occupied in ANY member: 0 on an
 *     occupied voxel, INT32_MAX everywhere when no member holds a voxel.  Integers throughout: the brute-force answer, the same bytes every time.
 *   info [2] int64 = {occupied voxels of the union, the largest finite d2 or -1}; the call sets both itself.
 * Three passes, along z, y and x, in place in d2: there is no workspace.
 *
 * 2. mnf_clearance_lookup.  points [n_points,3] float64 in the grid's axis order, trajectory t = points offsets[t] .. offsets[t+1]-1
 * (offsets [n_traj+1] int64, ascending from 0 to n_points; an offset outside [0, n_points] is clamped, so nothing outside the arrays is
 * touched).  origin_host three host doubles (aabb[:3]), voxel > 0.
 *   The voxel of a point is numpy's  (p_k - origin_k) // voxel  in float64, cast to int: q = fmod-exact floor division, that is
 *     mod = fmod(a, b); div = (a - mod) / b; if (mod != 0 and (b < 0) != (mod < 0)) div -= 1;
 *     q = div == 0 ? copysign(0, a / b) : (f = floor(div), div - f > 0.5 ? f + 1 : f)
 *   (1.0 // 0.2 is 4, not 5).  A quotient beyond +-2^30 is clamped there; one that is not finite gives INT32_MIN.
 *   cells [n_points,3] int32; point_d2 [n_points] int32 = d2 of the voxel, -1 for a voxel outside the grid or a point that is not finite.
 *   traj [n_traj,4] int64 = {the least point_d2 over the samples inside or -1, the index within the trajectory of the FIRST sample that
 *     attains it or -1, samples outside (the non-finite ones included), samples}.  The minimum is taken over integer keys
 *     (d2 << 32 | index): the same whatever the schedule.
 *   info [2] int64 += {samples outside, samples not finite}: the caller clears it.
 * Points that no trajectory covers are not looked at.  n_traj == 0 is a no-op.
 *
 * 3. mnf_voxel_walk_*: planning/planning_funcs.py:97-159, get_voxels_between_points(start_pos, end_pos, current_voxel, end_voxel,
 * voxel_size), every statement in float64 / int32 as numpy evaluates it.  start, end [n,3] float64; current_voxel, end_voxel [n,3] int32:
 * four separate arguments, as the function takes them, so a caller that mixes frames (collision_checker does) gets the reference's answer.
 *   step_k = ray_k >= 0 ? +1 : -1, ray = end - start;  next_k = (current_k + step_k) * voxel_size;
 *   t_max_k = (next_k - start_k) / ray_k, t_delta_k = voxel_size / ray_k * step_k, both inf where ray_k == 0;
 *   range_sq = dist(end_voxel), dist(v) = ((a + b) + c) of the squares of (v_k - current_k) * voxel_size;
 *   while dist(voxel) <= range_sq: step along x if t_max_x < t_max_y and t_max_x < t_max_z; along z if t_max_x < t_max_y otherwise; along y
 *   if t_max_y < t_max_z; else along z; add t_delta to that t_max; LIST the voxel.
 * So the start voxel is not listed, the walk overshoots the end voxel and may leave the grid, a negative direction crosses the far face
 * of the previous voxel first, and a zero-length ray takes one step in +z.  These are the reference's and are kept.
 * Every walk is bounded: one that would list more than max_steps (0 .. 2^31 - 1) voxels is cut there, and one with a start or end that is
 * not finite has length 0.  info [3] int64 += {walks cut, walks not finite, slots that did not match (fill only)}: the caller clears it.
 *   mnf_voxel_walk_count: counts [n] int64.
 *   mnf_voxel_walk_fill: voxels [total,3] int32, walk w at rows offsets[w] .. offsets[w+1]-1 (offsets [n+1] int64, the exclusive sum of the
 *     counts).  Nothing is written outside a walk's slot or outside [0, total); a walk whose length is not its slot is counted in info[2].
 *   mnf_voxel_walk_hits: hits [n,5] int32 = {position in the list of the first voxel occupied in any of the n_members grids or -1, that
 *     voxel's three indices as listed (unclipped; -1 each when there is none), the length of the list}.  Every index is clipped to the grid
 *     before the look-up, as collision_checker clips (planning_funcs.py:174-178).  No list is built.
 *
 * Argument errors (a null required pointer, a size outside the limits, a voxel size that is not positive and finite, an origin that is not
 * finite, a count or max_steps outside its range, an int64 or float64 array that is misaligned) return MNF_ERR_INVALID before any HIP call.
 * n == 0 is a no-op.  Profile labels: "clearance_field", "clearance_lookup", "voxel_walk_count", "voxel_walk_fill", "voxel_walk_hits".  Every
 * call enqueues on `stream` and none synchronises.  There is no CPU fallback. */
int mnf_clearance_field(const uint8_t *binaries, int32_t n_members, int32_t X, int32_t Y, int32_t Z, int32_t *d2, int64_t *info, mnf_stream_t stream);
int mnf_clearance_lookup(const int32_t *d2, int32_t X, int32_t Y, int32_t Z, const double *origin_host, double voxel, const double *points,
                         int64_t n_points, const int64_t *offsets, int64_t n_traj, int32_t *cells, int32_t *point_d2, int64_t *traj, int64_t *info,
                         mnf_stream_t stream);
int mnf_voxel_walk_count(const double *start, const double *end, const int32_t *current_voxel, const int32_t *end_voxel, int64_t n,
                         double voxel_size, int64_t max_steps, int64_t *counts, int64_t *info, mnf_stream_t stream);
int mnf_voxel_walk_fill(const double *start, const double *end, const int32_t *current_voxel, const int32_t *end_voxel, int64_t n,
                        double voxel_size, int64_t max_steps, const int64_t *offsets, int64_t total, int32_t *voxels, int64_t *info,
                        mnf_stream_t stream);
int mnf_voxel_walk_hits(const double *start, const double *end, const int32_t *current_voxel, const int32_t *end_voxel, int64_t n,
                        double voxel_size, int64_t max_steps, const uint8_t *binaries, int32_t n_members, int32_t X, int32_t Y, int32_t Z,
                        int32_t *hits, int64_t *info, mnf_stream_t stream);

/* ---------------------------------------------------------------- min-snap candidate trajectories */

/* The curve sample_traj (planning/planning_funcs.py:328-397) lays through a traced path, its samples and their view poses: the stretch between
 * mnf_path_trace and mnf_clearance_lookup.  Everything is float64; the unit is built without FMA contraction.  Motor speeds, moments, cmd_w,
 * cmd_a and the simulator are not restated: sample_traj uses cmd_q only.
 *
 * Trajectory t owns the waypoints offsets[t] .. offsets[t+1]-1 (offsets [n_traj+1] int64, ascending from 0 to n_waypoints; an offset outside
 * [0, n_waypoints] is clamped).  Every per-segment and per-keyframe output is packed at the SAME offsets: a trajectory of W waypoints has at
 * most W - 1 segments and W keyframes, so its segments are rows offsets[t] .. offsets[t] + n_segments[t] - 1 and its keyframes one more.  Rows
 * past those, and every row of a refused trajectory, are left untouched.
 *
 * 1. mnf_minsnap_solve <- trajectories/minsnap.py:254-371 (MinSnap.__init__, initialize).  Give `points` [n_waypoints,3] float64, or `cells`
 * [n_waypoints,2] int32 as mnf_path_trace lists them (goal first) with resolution, origin_host (three host doubles, aabb[:3]) and height: the
 * cells of a trajectory are reversed and become (cx * resolution + origin[0], cy * resolution + origin[1], height + origin[2]), the
 * reference's dij_waypoints (planning_funcs.py:328-340); the other of the two pointers is null.  In the reference's order of operations:
 *   seg_dist[k] = sqrt((dx dx + dy dy) + dz dz) between ALL consecutive waypoints; a waypoint is kept if it is the first or seg_dist > 1e-2;
 *   m = kept - 1;  total = np.sum(seg_dist) (numpy's pairwise order);  for i < m: cum += seg_dist[i] (the UNMASKED distances, as the
 *   reference indexes them), vf = min(min(cum, v_avg), total - cum), delta_t[i] = seg_dist[i] * 2 / (vf + vi + 1e-4), vi = vf;
 *   t_keyframes = {0, the sequential running sum of delta_t};  yaw_execute = t_keyframes / (t_keyframes[m] + 1e-4) * (yaw1 - yaw0) + yaw0
 *   (sample_traj's np.linspace(2 pi, 0, n) enters the reference by its two ends only).
 * The reference solves no QP: its curve is the solution of the square system A c = b of get_1d_equality_constraints (minsnap.py:63-245),
 * the same A for x, y, z and yaw.  With the three start rows first, then per segment its two position rows and its six continuity rows, then
 * the three end rows, A has lower and upper bandwidth 4.  The call assembles that band from delta_t (powers by repeated multiplication) and
 * eliminates it with partial pivoting over the four right-hand sides; factored rows go through `workspace`.
 *   coeffs [n_waypoints][4][8]: segment row, axis (x, y, z, yaw), power, LOWEST first, as c_opt holds them.
 *   delta_t, t_keyframes, yaw_execute [n_waypoints];  n_segments [n_traj] int32 = m;  status [n_traj] int32:
 *     MNF_MINSNAP_OK               a curve was written.
 *     MNF_MINSNAP_NULL             one waypoint is left (or the trajectory is empty): the reference's `null`.  No curve, no samples.
 *     MNF_MINSNAP_REJECTED_SHORT   two waypoints are left: the reference's time allocation gives that lone segment 2 d / 1e-4 seconds and
 *                                  its rank test refuses the system (rank 3 of 8), always.  No curve, no samples.
 *     MNF_MINSNAP_SINGULAR         a pivot fell below 8 m * eps * |A|_inf, a delta_t was not positive, or a coefficient is not finite.
 *                                  THIS PROJECT'S criterion: the reference's SVD rank test is not reproduced.  From two segments on every
 *                                  delta_t of a grid path is bounded and both accept.
 *     MNF_MINSNAP_TOO_LONG         more than MNF_MINSNAP_MAX_SEGMENTS segments, or more than 4096 waypoints before the mask.
 *     MNF_MINSNAP_NOT_FINITE       a waypoint is not finite.
 *
 * 2. mnf_minsnap_sample_count <- planning_funcs.py:352-370.  For every trajectory with status OK: t_final = np.sum(delta_t),
 * N = max(int(t_final * rate), min_samples), t_step = t_final / N, and the sample times 0, then t_k = t_{k-1} + t_step as a sequential float64
 * running sum, the last being the first with t_k >= t_final (N + 1 or N + 2 of them: the sum may fall an ulp short).  counts [n_traj] int64;
 * the times are left in the workspace, max_samples per trajectory, for the fill.  A trajectory with more than max_samples samples gets count 0
 * and sample_status MNF_MINSNAP_SAMPLE_OVERFLOW (MNF_MINSNAP_SAMPLE_INVALID for a trajectory record that contradicts itself); a refused
 * trajectory gets count 0.  sample_status [n_traj] int32.
 *
 * 3. mnf_minsnap_sample_fill, with the same workspace, untouched since the count.  sample_offsets [n_traj+1] = the exclusive sum of counts,
 * n_samples its last entry; pose_offsets [n_traj+1] = the exclusive sum of (count ? count + n_look : 0), n_poses its last entry.  Per sample
 * <- minsnap.py:386-443 (update): t clipped to the keyframes, the first segment i with t_keyframes[i] + delta_t[i] >= t, Horner as np.polyval,
 * derivative coefficients by np.polyder's successive integer multiples; quadrotor_control.py:104-124, :177: b3 = normalize(x_ddot + (0, 0,
 * 9.81)), c1 = (cos yaw, sin yaw, 0), b2 = normalize(b3 x c1), b1 = b2 x b3, the quaternion (x, y, z, w) of R = [b1 b2 b3] by scipy's
 * largest-of-diagonal-and-trace rule; planning_funcs.py:377-386: from_rotvec(P as_rotvec(q)) in closed form = (-x, z, -y, w) of q with the
 * sign that makes w >= 0.
 *   flat_x [n_samples,3] = flat["x"] (the planner's x, y, height);  times [n_samples];
 *   derivatives [n_samples,12] = x_dot, x_ddot, x_dddot, x_ddddot (or null);  yaw [n_samples,3] = yaw, yaw_dot, yaw_ddot (or null);
 *   poses [n_poses,7] = (x, height, y) + quaternion per sample, then n_look rows of the LAST sample's position with look_quats [n_look,4], the
 *   caller's table (planning_funcs.py:391-395).
 * A trajectory whose two slots do not agree with each other is left untouched; nothing is written outside [0, n_samples) and [0, n_poses).
 *
 * mnf_minsnap_workspace_bytes(n_traj, n_waypoints, max_samples): what any of the three calls needs (840 bytes per waypoint for the solve,
 * 8 n_traj max_samples for the samples, the larger of the two), or -1 for a size outside [0, 2^31).
 * Argument errors return MNF_ERR_INVALID before any HIP call.  n_traj == 0 is a no-op.  Profile labels: "minsnap_solve",
 * "minsnap_sample_count", "minsnap_sample_fill".  Every call enqueues on `stream` and none synchronises.  There is no CPU fallback. */
#define MNF_MINSNAP_MAX_SEGMENTS 1023
#define MNF_MINSNAP_OK 0
#define MNF_MINSNAP_NULL 1
#define MNF_MINSNAP_REJECTED_SHORT 2
#define MNF_MINSNAP_SINGULAR 4
#define MNF_MINSNAP_TOO_LONG 8
#define MNF_MINSNAP_NOT_FINITE 16
#define MNF_MINSNAP_SAMPLE_OVERFLOW 32
#define MNF_MINSNAP_SAMPLE_INVALID 64
int64_t mnf_minsnap_workspace_bytes(int64_t n_traj, int64_t n_waypoints, int64_t max_samples);
int mnf_minsnap_solve(const double *points, const int32_t *cells, const int64_t *offsets, int64_t n_traj, int64_t n_waypoints, double resolution,
                      const double *origin_host, double height, double yaw0, double yaw1, double v_avg, double *coeffs, double *delta_t,
                      double *t_keyframes, double *yaw_execute, int32_t *n_segments, int32_t *status, void *workspace, int64_t workspace_bytes,
                      mnf_stream_t stream);
int mnf_minsnap_sample_count(const double *delta_t, const int64_t *offsets, int64_t n_waypoints, const int32_t *n_segments, const int32_t *status,
                             int64_t n_traj, double rate, int64_t min_samples, int64_t max_samples, int64_t *counts, int32_t *sample_status,
                             void *workspace, int64_t workspace_bytes, mnf_stream_t stream);
int mnf_minsnap_sample_fill(const double *coeffs, const double *delta_t, const double *t_keyframes, const int64_t *offsets, int64_t n_waypoints,
                            const int32_t *n_segments, int64_t n_traj, int64_t max_samples, const int64_t *sample_offsets, int64_t n_samples,
                            const int64_t *pose_offsets, int64_t n_poses, const double *look_quats, int32_t n_look, double *flat_x, double *times,
                            double *derivatives, double *yaw, double *poses, const void *workspace, int64_t workspace_bytes, mnf_stream_t stream);

/* ---------------------------------------------------------------- scene sensor */

/* What the reference takes from habitat_sim (simulator/sim.py:169-196, HabitatSim.sample_images_from_poses): colour, planar depth and class
 * images of a ground-truth world at given poses.  The world here is a labelled, coloured voxel grid; one launch renders a batch of poses and
 * the images stay on the device.  This comment is the definition: every output byte follows from it (tests/sensor_ref.py restates it).
 *
 * Scene.  voxels [X][Y][Z] uint32, lin = (x Y + y) Z + z, the estimator's layout.  Bits 0-7, 8-15, 16-23 of a word are r, g, b; bits 24-31
 * the class; class 0xFF means FREE (the colour bits of a free voxel mean nothing).  The grid's origin lo_host (three host doubles) and the
 * voxel edge voxel_size (> 0) are host float64.  The brick mask `bricks` holds one bit per 8 x 8 x 8 brick, set where any voxel of the
 * brick is occupied: a one-plane bit grid over ceil(X/8) x ceil(Y/8) x ceil(Z/8) bricks laid out as every bit grid here (brick
 * (bx, by, bz) is bit (b & 31) of word b >> 5, b = (bx BY + by) BZ + bz; the word count is rounded up to even).
 *   mnf_sensor_bricks_words(X, Y, Z): the words of the mask, or -1 for a scene outside the limits.
 *   mnf_sensor_build_bricks: clears the mask and fills it from voxels, on `stream`.
 * Limits: those of a bit grid (axes <= 2^24, X Y Z < 2^31 - 64) and a mask of at most 16384 words = 64 KiB, which a workgroup stages in LDS
 * (524288 bricks: 540 x 84 x 560 voxels take 1638 words).  A caller that edits voxels rebuilds the mask; a mask with a bit missing hides
 * that brick's voxels, a bit too many costs time only.
 *
 * The walk, in float64, every operation rounded separately (the unit is built without FMA contraction).  A ray is o + t d, t >= 0, d NOT
 * normalised, limited to near <= t <= far (0 <= near <= far, far finite).  With N = (X, Y, Z) and a = 0, 1, 2:
 *   g_a = (o_a - lo_a) / s,  e_a = d_a / s,  step_a = sign(e_a) (0 for e_a = 0),  inv_a = 1 / e_a.
 *   A ray with an o_a, d_a, g_a or e_a that is not finite is a MISS and is counted as not finite.
 *   Box: for step_a != 0, t0_a = ((step_a > 0 ? 0 : N_a) - g_a) inv_a and t1_a the same with the other face; for step_a = 0 the ray misses
 *   unless 0 <= g_a < N_a.  t_in = near, face 6; then for a = 0, 1, 2: if t0_a > t_in, t_in = t0_a and face = 2 a + (step_a < 0).
 *   t_out = the least of far and the t1_a.  The ray misses unless t_in <= t_out.
 *   Start: c_a = clamp(floor(g_a + e_a t_in), 0, N_a - 1), t = t_in.
 *   Loop: if voxel c is occupied: HIT, t_hit = max(t, t_in), the voxel lin(c), the face as last set.  Otherwise
 *     f_a = ((c_a + (step_a > 0)) - g_a) inv_a (+inf where step_a = 0); a = the axis of the least f_a, the lowest on a tie (a = 0; if
 *     f_1 < f_a, a = 1; if f_2 < f_a, a = 2); the ray misses unless f_a <= t_out; c_a += step_a and the ray misses if that leaves the
 *     grid; t = f_a, face = 2 a + (step_a < 0).
 * f_a is formed from the integer cell every time and never accumulated: a monotone function of c_a, so the walk cannot drift, and it ends
 * after at most X + Y + Z steps.  Faces: 0 / 1 the voxel's low / high x face (the ray came in moving towards +x / -x), 2 / 3 for y, 4 / 5
 * for z, 6 the near plane (the ray started inside the voxel), 255 no hit.
 *
 * mnf_sensor_cast_rays.  origins, dirs [n,3] float64 -> t_hit [n] float64 (-1 on a miss), hit [n] int32 (lin or -1), face [n] uint8.
 *
 * mnf_sensor_views.  c2w [n_views][3][4] float64 (rotation columns and position), a pinhole camera looking along -z as the dataset's
 * (habitat_to_data.py:274-301), pixel (x, y) of a width x height image, in the order mnf_generate_rays uses but in float64:
 *   cam = (((x - width/2) + 0.5) / focal, ((y - height/2) + 0.5) / focal * (-1), -1);  d_i = (cam_0 R_i0 + cam_1 R_i1) + cam_2 R_i2;  o = c2w[:, 3].
 *   rgba  [n_views][height][width][4] uint8: channel k = (c_k shade[face] + 127) / 255 in integers, alpha 255; shade_host is seven host bytes,
 *         one per face 0 .. 6.  A miss gets `background` (r in bits 0-7, g 8-15, b 16-23, alpha 24-31).  One 32-bit store per pixel.
 *   depth [n_views][height][width] float32: MNF_SENSOR_DEPTH_PLANAR: (float)t_hit, since cam_2 = -1 makes t the distance along the
 *         camera's axis, Habitat's depth; MNF_SENSOR_DEPTH_RAY: (float)(t_hit sqrt((cam_0 cam_0 + cam_1 cam_1) + 1)), the length along the
 *         normalised ray of the dataset.  0 on a miss.
 *   sem   [n_views][height][width] uint8: the voxel's class; 0 on a miss.
 *   hit   [n_views][height][width] int32 or null: lin or -1.
 * info [2] int64 += {misses (the rays that are not finite included), rays not finite}: the caller clears it (both calls).
 *
 * Argument errors (a null required pointer, a scene outside the limits, an origin, voxel size, focal, near or far outside its range, an
 * image wider or higher than 16384, an unknown depth_mode, a misaligned array) return MNF_ERR_INVALID before any HIP call.  n == 0 and
 * n_views == 0 are no-ops.  Profile labels: "sensor_build_bricks", "sensor_cast_rays", "sensor_views".  Every call enqueues on `stream` and
 * none synchronises.  There is no CPU fallback. */
#define MNF_SENSOR_DEPTH_PLANAR 0
#define MNF_SENSOR_DEPTH_RAY 1
int64_t mnf_sensor_bricks_words(int32_t X, int32_t Y, int32_t Z);
int mnf_sensor_build_bricks(const uint32_t *voxels, int32_t X, int32_t Y, int32_t Z, uint32_t *bricks, mnf_stream_t stream);
int mnf_sensor_cast_rays(const uint32_t *voxels, int32_t X, int32_t Y, int32_t Z, const uint32_t *bricks, const double *lo_host, double voxel_size,
                         const double *origins, const double *dirs, int64_t n, double near, double far, double *t_hit, int32_t *hit, uint8_t *face,
                         int64_t *info, mnf_stream_t stream);
int mnf_sensor_views(const uint32_t *voxels, int32_t X, int32_t Y, int32_t Z, const uint32_t *bricks, const double *lo_host, double voxel_size,
                     const double *c2w, int32_t n_views, int32_t width, int32_t height, double focal, double near, double far, int32_t depth_mode,
                     const uint8_t *shade_host, uint32_t background, uint8_t *rgba, float *depth, uint8_t *sem, int32_t *hit, int64_t *info,
                     mnf_stream_t stream);

/* ---------------------------------------------------------------- pose refinement against the frozen map (csrc/localize.hip)
 *
 * State estimation for a capture whose pose comes from odometry: B views of the dataset, each with its own correction xi[b] = (rotvec [3] axis-angle,
 * trans [3]) of its initial pose c2w0[b], refined against the field with its parameters frozen (iNeRF-style).  What render.transform_rays +
 * fused_train_render_rays + torch.optim.Adam do for one view and one iteration per host round, here for B views and a whole run of iterations in ONE C call
 * that never synchronises.  xi and Adam's two moments adam_m, adam_v are float64 [B,6] on the device and stay there between calls.
 *
 * mnf_pose_rays.  Rays and targets of B views x n rays (ray i = b n + r).
 *   Pixel: pix_idx[b n + r] (flat id y W + x, int64; clamped into the image) or, with pix_idx NULL, drawn: (u0, u1, .., ..) = Philox4x32-10 of counter
 *     (r, b, iteration, 0x706F7365) with key (seed low, seed high); x = (u0 W) >> 32, y = (u1 H) >> 32 in 64-bit integers, pix = y W + x.  pix_out [B,n]
 *     receives the ids either way.
 *   Ray: d = mnf_generate_rays' direction of that pixel from c2w0[b] ([B,3,4] f32), in its fp32 operation order.  R = I + a K + b K^2 of rotvec in float64
 *     (a = sin t / t, b = (1 - cos t) / t^2, t = |rotvec|; below t^2 = 1e-6 the series a = 1 - t^2/6 + t^4/120, b = 1/2 - t^2/24 + t^4/720: transform_rays'
 *     branches), rounded ONCE to fp32 (rot_out [B,9], optional).  d' = ((R_j0 d_0 + R_j1 d_1) + R_j2 d_2)_j in fp32;  o' = (float)((double)c + trans), c the
 *     camera centre c2w0[b][:,3]: every ray of a view starts there, so transform_rays' rotation about the common origin drops out.
 *   Targets: mnf_gather_pixels' of image image_ids[b] (device int64 [B], clamped to [0, n_images)) for either storage layout: target_rgb [B n,3] f32,
 *     target_depth [B n] f32, target_label [B n] int64.
 *
 * mnf_pose_loss.  Per view b, from the four rendered planes of its n rays:  loss[b] = w_rgb mean smooth_l1(rgb - target_rgb) + w_dep mean
 *   smooth_l1(depth - target_depth) + w_sem mean CE(sem, target_label)  (pipeline.py:506-511's forms; every mean over the VIEW's own rays; float64 [B]), and
 *   its gradients g_rgb [B n,3], g_depth [B n], g_sem [B n,C] (fp32, dense: what mnf_train_render_backward_rays reads with strides (3,1), 1, (C,1)).  A label
 *   outside [0, C) in a view sets view_status[b] = 8 (else 0), ORs 8 into *status_word (optional) and zeroes that view's gradients; such a ray adds nothing
 *   to the loss.  n_classes 0: no semantic term, sem / g_sem may be NULL.  One workgroup per view, sums in a fixed order.
 *
 * mnf_pose_update.  Per view, one workgroup:  S_o = sum_r g_rays_o[r],  S_w = sum_r rays_d[r] x g_rays_d[r]  over the view's rays in float64 in a fixed
 *   order (no atomics: the same inputs give the same bytes);  dL/dtrans = S_o,  dL/drotvec = J_l(rotvec)^T S_w,  J_l = I + b K + c K^2,
 *   b = (1 - cos t) / t^2, c = (t - sin t) / t^3 (below t^2 = 1e-6: b = 1/2 - t^2/24 + t^4/720, c = 1/6 - t^2/120 + t^4/5040);  grad_out [B,6]
 *   (optional) receives (dL/drotvec, dL/dtrans).  Then one Adam step on the six numbers: learning rates lr_rot / lr_trans, bias-corrected moments, the
 *   view's step number iteration + 1 - stalled[b].  A view is LEFT ALONE — xi and moments untouched, stalled[b] += 1 — when none of its rays kept a sample
 *   (kept_cnts [B n] int64; NULL: every ray counts as kept), when view_status[b] != 0 (NULL: none), when *skip_dev > 0 (NULL: never), or when its gradient
 *   is not finite.  `stalled` is cumulative over a refinement: the caller zeroes it once, with xi and the moments.
 *
 * mnf_pose_refine.  For iteration first_iter + it, it = 0 .. n_iters - 1, enqueues in order: mnf_pose_rays; mnf_train_render_forward's launches on all B n
 *   rays (the caller's `opts` with stratified = 0 and presampled = NULL: the sample set is a constant of each render, no gradient passes through the sample
 *   positions); mnf_pose_loss; mnf_train_render_backward_rays' launches with the three parameter pointers NULL (frozen: the field's parameters are read, never
 *   written); mnf_pose_update with the forward's per-ray kept counts, the loss' view bits and the render's skip flag (a sample bound exceeded, a ray past the
 *   scratch row, no sample at all, a non-finite gradient).  loss_trace [n_iters,B] float64 and counts_dev [n_iters,4] int64 (mnf_train_step's four counters
 *   of each iteration's render; a bad label ORs 8 into its status word) are indexed from THIS call's first iteration.  After status bit 1 or 4 the caller
 *   raises max_marched / max_kept and calls again: the views stalled meanwhile.  No hand-over to the call-by-call route happens inside: at most four
 *   occupancy levels, no ray past the scratch row (status bit 2 stalls every view).  workspace: mnf_pose_refine_workspace_bytes(f, n_views, rays_per_view,
 *   max_marched, max_kept) device bytes, 256-byte aligned; mnf_pose_refine_workspace_offset gives the byte offset of what the LAST iteration left there
 *   (MNF_POSE_WS_*: rays [B n,3], pixel ids, the four planes, the ray gradients, the 6-vector gradients [B,6] f64, R [B,9] f32, the render's
 *   kept-sample count of every ray [B n] int64), for tests and tools.
 *
 * mnf_pose_opts starts with struct_size (MNF_INIT).  Argument errors (a null required pointer, a wrong struct_size, sizes <= 0 or B n > 2^31 - 1, a
 * misaligned float64 / int64 array, learning rates < 0, betas outside [0, 1), eps <= 0) return MNF_ERR_INVALID before any HIP call; a NULL or short workspace
 * MNF_ERR_WORKSPACE.  Profile labels: "pose_rays", "pose_loss", "pose_update".  Every call enqueues on `stream`, none synchronises.  There is no CPU fallback. */
typedef struct mnf_pose_opts_s {
    uint32_t struct_size;          /* sizeof(mnf_pose_opts) */
    float w_rgb, w_dep, w_sem;     /* the loss weights (pipeline.py:511: 10, 1/5, 1/2) */
    double lr_rot, lr_trans;       /* Adam's learning rate for rotvec and for trans */
    double beta1, beta2, eps;      /* Adam (the project's optimizers: 0.9, 0.999, 1e-15) */
    uint64_t seed;                 /* key of the pixel draw */
} mnf_pose_opts;
#define MNF_POSE_WS_RAYS_O 0
#define MNF_POSE_WS_RAYS_D 1
#define MNF_POSE_WS_PIX 2
#define MNF_POSE_WS_RGB 3
#define MNF_POSE_WS_ACC 4
#define MNF_POSE_WS_DEPTH 5
#define MNF_POSE_WS_SEM 6
#define MNF_POSE_WS_G_RAYS_O 7
#define MNF_POSE_WS_G_RAYS_D 8
#define MNF_POSE_WS_GRAD 9
#define MNF_POSE_WS_ROT 10
#define MNF_POSE_WS_KEPT 11
int mnf_pose_rays(const uint8_t *images, const void *depths, int32_t depth_is_f16, const void *semantics, int32_t sem_is_u8, int64_t n_images,
                  const int64_t *image_ids, const float *c2w0, float focal, int32_t width, int32_t height, const int64_t *pix_idx, const double *xi,
                  int32_t n_views, int32_t rays_per_view, int64_t iteration, uint64_t seed, float *rays_o, float *rays_d, int64_t *pix_out, float *rot_out,
                  float *target_rgb, float *target_depth, int64_t *target_label, mnf_stream_t stream);
int mnf_pose_loss(const float *rgb, const float *depth, const float *sem, const float *target_rgb, const float *target_depth, const int64_t *target_label,
                  int32_t n_views, int32_t rays_per_view, int32_t n_classes, const mnf_pose_opts *pose, double *loss, float *g_rgb, float *g_depth, float *g_sem,
                  int32_t *view_status, int64_t *status_word, mnf_stream_t stream);
int mnf_pose_update(const float *g_rays_o, const float *g_rays_d, const float *rays_d, const int64_t *kept_cnts, const int32_t *view_status,
                    const int32_t *skip_dev, int32_t n_views, int32_t rays_per_view, int64_t iteration, const mnf_pose_opts *pose, double *xi, double *adam_m,
                    double *adam_v, int32_t *stalled, double *grad_out, mnf_stream_t stream);
int64_t mnf_pose_refine_workspace_bytes(mnf_field_t f, int32_t n_views, int32_t rays_per_view, int64_t max_marched, int64_t max_kept);
int64_t mnf_pose_refine_workspace_offset(mnf_field_t f, int32_t n_views, int32_t rays_per_view, int64_t max_marched, int64_t max_kept, int32_t what);
int mnf_pose_refine(mnf_field_t f, const uint8_t *binaries, const uint32_t *bitgrid, const float *occs, int32_t res_x, int32_t res_y, int32_t res_z,
                    const float *aabb_host, const uint8_t *images, const void *depths, int32_t depth_is_f16, const void *semantics, int32_t sem_is_u8,
                    int64_t n_images, const int64_t *image_ids, const float *c2w0, float focal, int32_t width, int32_t height, const int64_t *pix_idx,
                    int32_t n_views, int32_t rays_per_view, double *xi, double *adam_m, double *adam_v, int64_t first_iter, int32_t n_iters,
                    const mnf_train_opts *opts, const mnf_pose_opts *pose, double *loss_trace, int32_t *stalled, int64_t *counts_dev, int64_t max_marched,
                    int64_t max_kept, void *workspace, int64_t workspace_bytes, mnf_stream_t stream);

/* ---------------------------------------------------------------- TSDF fusion of captures (csrc/tsdf.hip)
 *
 * The classical map any robotics stack builds from the same captures the field is trained on: a truncated signed distance volume fused
 * from depth, colour and class images (Curless & Levoy 1996; KinectFusion), its lattice for mnf_surface_extract_observed, and the colour
 * and class of mesh vertices.  This comment is the definition: every output byte follows from it (tests/tsdf_ref.py restates it).
 *
 * Volume.  Lattice points [X+1][Y+1][Z+1] with X = cells_x etc. (1 .. 1024 each), lin(p) = (x (Y+1) + y)(Z+1) + z, exactly the lattice of
 * mnf_surface_extract; point i of an axis is at w = lo + (double)i * voxel (lo_host three host doubles, voxel a host double).  The state is
 * four device arrays of one element per point, 16 bytes per point:
 *   tsdf   f32    the running mean of min(1, sdf / trunc); 1 for a point never observed (the caller's initial value)
 *   weight int32  observations so far, capped at max_weight; initially 0
 *   word   uint32 r | g << 8 | b << 16 | class << 24 of one observation (the sensor's voxel word); initially anything
 *   best   f32    the |sdf| of the observation that wrote `word`; -1 for none
 *
 * mnf_tsdf_integrate applies views 0 .. n_views - 1 in ascending order to every lattice point.  A view is c2w [3][4] float64 (rotation
 * columns and position c, as mnf_sensor_views takes it) of a pinhole camera looking along -z with a double `focal` and width x height
 * pixels; depth [n_views][height][width] is f32 (MNF_TSDF_DEPTH_F32) or f16 (MNF_TSDF_DEPTH_F16); colour uint8
 * [n_views][height][width][colour_stride], colour_stride 3 or 4 (bytes 0..2 are r, g, b); classes uint8 (MNF_TSDF_CLASS_U8) or int64
 * (MNF_TSDF_CLASS_I64) [n_views][height][width].  depth_mode is MNF_SENSOR_DEPTH_PLANAR (the depth is the distance along the camera's axis)
 * or MNF_SENSOR_DEPTH_RAY (the length of the pixel's ray).  For a point and a view, in float64, every operation rounded separately (the
 * unit is built without FMA contraction):
 *    1. q_k = w_k - c_k.
 *    2. xc = (q_0 R_00 + q_1 R_10) + q_2 R_20;  yc = (q_0 R_01 + q_1 R_11) + q_2 R_21;  zc = (q_0 R_02 + q_1 R_12) + q_2 R_22.
 *    3. zd = -zc.  The view is SKIPPED unless zd > min_depth.
 *    4. u = floor((xc / zd) * focal + (double)width * 0.5),  v = floor(((-yc) / zd) * focal + (double)height * 0.5): the inverse of the sensor's
 *       pixel-centre convention.  Skipped unless 0 <= u < width and 0 <= v < height (a NaN fails); px = (int)u, py = (int)v.
 *    5. d = the stored depth of pixel (py, px), widened exactly.  Skipped and counted (info[2]) when d is not finite, d <= 0 or d > max_depth.
 *    6. along = zd (planar) or sqrt((q_0 q_0 + q_1 q_1) + q_2 q_2) (ray).
 *    7. sdf = d - along.  Skipped and counted (info[3]) when sdf < -trunc.
 *    8. s = min(1, sdf / trunc).
 *    9. tsdf = (float)(((double)tsdf * (double)weight + s) / (double)(weight + 1)), with the weight BEFORE the update; info[0] counts the
 *       observation, info[1] too when that weight was 0.
 *   10. weight = min(weight + 1, max_weight).
 *   11. With a = |sdf|: when a <= trunc and (best < 0 or (float)a < best): best = (float)a and word = the pixel's r, g, b and class.
 *   12. A class outside [0, 255] (int64 layout) stores 255 and is counted (info[4]) each time such a word is stored.
 * Nearest pixel, no interpolation; one truncation for the whole volume; colour and class are those of the observation closest to the
 * surface, not an average.
 * info [5] int64 += {observations applied, points observed for the first time, invalid depths, observations behind the surface, labels out
 * of range}: the caller clears it.  Only these are counted: none depends on how a kernel culls (a kernel may skip only work that changes
 * nothing: a view that misses the volume leaves every byte and every counter as it was; there is no cull on max_depth, because a far point
 * that projects onto a pixel still counts as behind the surface or as an invalid depth).  No atomics touch the state: the same inputs give
 * the same bytes, and n_views views in one call give the bytes of n_views calls of one view each, in order.  The state arrays must not
 * overlap the images.
 *
 * mnf_tsdf_lattice.  values [X+1][Y+1][Z+1] f32: -tsdf where weight >= min_weight (>= 1), else NaN: inside (value > 0) is behind a surface,
 * the iso-surface at 0 is the fused surface, NaN is UNOBSERVED (mnf_surface_extract_observed).  counts [3] int64 (overwritten) = {points with
 * weight >= min_weight, those of them with tsdf < 0, points with best >= 0}.
 *
 * mnf_tsdf_vertex_attrs.  positions [n][3] f32 -> colour [n][3] uint8, label [n] int32 and, with a palette [n_palette][3] uint8,
 * sem_colour [n][3] uint8 (any output may be NULL).  The cell of a vertex is c_k = floor(((double)pos_k - lo_k) / voxel) per axis in
 * float64, clamped into 0 .. cells_k - 1 (a NaN gives 0).  Of the cell's 8 corners the one with best >= 0 and the smallest best gives its
 * word (ties go to the lowest lin): colour = its r, g, b, label = its class byte, sem_colour = palette[label], or (0,0,0) where label >=
 * n_palette.  With no such corner: colour 0, label -1, sem_colour 0.
 *
 * mnf_surface_extract_observed (csrc/surface.hip): mnf_surface_extract with ONE rule changed.  A NaN lattice point is UNOBSERVED rather
 * than outside: an edge carries a vertex only when its ends differ in inside-ness AND neither end is NaN; a tetrahedron emits its triangles
 * only when none of its four vertices is NaN.  Order, arithmetic, normals, capacities, workspace and info are those of mnf_surface_extract,
 * and on a lattice without NaN the outputs are the same bytes.  A vertex that no triangle uses may remain (an edge between two observed
 * points all of whose tetrahedra hold an unobserved one).  The mesh is open where nothing was observed.  The unchanged entry would wrap
 * every observed region of a TSDF lattice in a shell of midpoint vertices.
 *
 * Argument errors (a null required pointer, cells outside 1 .. 1024, a lo, voxel, trunc or focal that is not finite or (the last three) not
 * positive, min_depth negative or not finite, max_depth not above min_depth or not finite, max_weight or min_weight outside 1 .. 2^31 - 1,
 * more than 65535 views or fewer than 0, an image wider or higher than 16384, a colour_stride other than 3 or 4, an unknown depth_type,
 * class_type or depth_mode, a misaligned array, n outside [0, 2^31)) return MNF_ERR_INVALID before any HIP call.  n_views == 0 and n == 0
 * return MNF_OK and do nothing.  Profile labels: "tsdf_integrate", "tsdf_lattice", "tsdf_vertex_attrs", "surface_extract_observed".  Every
 * call enqueues on `stream` and none synchronises.  There is no CPU fallback. */
#define MNF_TSDF_DEPTH_F32 0
#define MNF_TSDF_DEPTH_F16 1
#define MNF_TSDF_CLASS_U8 0
#define MNF_TSDF_CLASS_I64 1
#define MNF_TSDF_MAX_VIEWS 65535
int mnf_tsdf_integrate(float *tsdf, int32_t *weight, uint32_t *word, float *best, int32_t cells_x, int32_t cells_y, int32_t cells_z,
                       const double *lo_host, double voxel, double trunc, int32_t max_weight, double min_depth, double max_depth, const double *c2w,
                       int32_t n_views, int32_t width, int32_t height, double focal, const void *depth, int32_t depth_type, const uint8_t *colour,
                       int32_t colour_stride, const void *classes, int32_t class_type, int32_t depth_mode, int64_t *info, mnf_stream_t stream);
int mnf_tsdf_lattice(const float *tsdf, const int32_t *weight, const float *best, int32_t cells_x, int32_t cells_y, int32_t cells_z,
                     int32_t min_weight, float *values, int64_t *counts, mnf_stream_t stream);
int mnf_tsdf_vertex_attrs(const uint32_t *word, const float *best, int32_t cells_x, int32_t cells_y, int32_t cells_z, const double *lo_host,
                          double voxel, const float *positions, int64_t n, const uint8_t *palette, int32_t n_palette, uint8_t *colour, int32_t *label,
                          uint8_t *sem_colour, mnf_stream_t stream);
int mnf_surface_extract_observed(const float *values, int32_t cells_x, int32_t cells_y, int32_t cells_z, float iso, const float *origin_host,
                                 const float *step_host, int64_t max_vertices, int64_t max_triangles, float *positions, float *normals,
                                 int32_t *triangles, int64_t *info, void *workspace, int64_t workspace_bytes, mnf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
