// The radiance-field handle and the C entry points of the field forward, compiled once: level table and fragment gather table (host arithmetic), handle
// create / destroy / queries, and the entry points that fill a FieldIO and hand it to the operand-type unit (field.hip: kernels, launch_field_impl,
// set_params_impl) through the handle's mfma_bf16 flag.  No kernel and no diagnostic knob lives here.
#include <cmath>
#include <cstring>

#include "field.h"

namespace mnf {

// ------------------------------------------------------------------ level table and fragment gather table
static int grid_levels(const mnf_field_config &cfg, LevelMeta *levels, int64_t *total) {
    const double pls = std::exp((std::log((double)cfg.max_resolution) - std::log((double)cfg.base_resolution)) / (cfg.n_levels - 1));
    const double log2_pls = std::log2(pls);
    int64_t offset = 0;
    for (int l = 0; l < cfg.n_levels; ++l) {
        const float scale = (float)(std::exp2(l * log2_pls) * cfg.base_resolution - 1.0);
        const uint32_t res = (uint32_t)std::ceil((double)scale) + 1u;
        const uint64_t dense = (uint64_t)res * res * res;
        uint64_t n = ((dense + 7) / 8) * 8;
        const uint64_t cap = 1ull << cfg.log2_hashmap_size;
        if (n > cap) n = cap;
        levels[l].scale = scale;
        levels[l].res = res;
        levels[l].size = (uint32_t)n;
        levels[l].offset = (uint32_t)offset;
        levels[l].hashed = dense > n ? 1u : 0u;
        {   // round-up magic number for an exact, branch-free unsigned division by n (33-bit multiplier form)
            const uint32_t d = (uint32_t)n;
            uint32_t fl = 31; while (!((d >> fl) & 1u)) --fl;
            if ((d & (d - 1)) == 0) { levels[l].div_magic = 0; levels[l].div_shift = fl - 1; }
            else {
                const uint64_t num = 1ull << (32 + fl);
                uint32_t pm = (uint32_t)(num / d);
                const uint64_t rem = num % d;
                pm += pm;
                const uint64_t twice = rem + rem;
                if (twice >= d) pm += 1;
                levels[l].div_magic = pm + 1; levels[l].div_shift = fl;
            }
        }
        offset += (int64_t)n;
    }
    *total = offset;
    return MNF_OK;
}

enum KMap { K_NATURAL, K_ACC, K_GEO };

// Append the fragment blocks of one [n_out_real x n_in_real] matrix (row-major [out][in], at `off` in buffer `buf`).
static void append_matrix(std::vector<int32_t> &t, int buf, int64_t off, int n_out_real, int n_in_real, int row_tiles,
                          const std::vector<std::pair<KMap, int>> &ksteps, int geo_base, int pad_col) {
    for (int rt = 0; rt < row_tiles; ++rt)
        for (size_t ks = 0; ks < ksteps.size(); ++ks)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 8; ++j) {
                    const int r = lane & 31, h = lane >> 5;
                    const int n = 32 * rt + r;
                    int k = -1;
                    const KMap km = ksteps[ks].first;
                    const int kb = ksteps[ks].second;
                    if (km == K_NATURAL) k = kb + 8 * h + j;
                    else if (km == K_ACC) k = kb + 8 * (j >> 2) + 4 * h + (j & 3);
                    else {
                        const int row = 8 * (j >> 2) + 4 * h + (j & 3);
                        k = row == 0 ? pad_col : geo_base + row - 1;
                    }
                    int32_t v = -1;
                    if (n < n_out_real && k >= 0 && k < n_in_real) v = (int32_t)((buf << 28) | (int32_t)(off + (int64_t)n * n_in_real + k));
                    t.push_back(v);
                }
}

static std::vector<std::pair<KMap, int>> acc_ksteps(int width) {
    std::vector<std::pair<KMap, int>> v;
    for (int k = 0; k < width; k += 16) v.push_back({K_ACC, (k / 32) * 32 + ((k / 16) & 1) * 16});
    return v;
}

static std::vector<int32_t> build_frag_table(const mnf_field_config &cfg) {
    const int W = cfg.neurons, Wh = W / 2, NH = cfg.layers;
    const int sem_pad = ((cfg.num_semantic_classes + 15) / 16) * 16;
    std::vector<int32_t> t;
    int64_t off = 0;
    // mlp_base: [W][64], (NH-1) x [W][W], [16][W]
    std::vector<std::pair<KMap, int>> nat64;
    for (int k = 0; k < 64; k += 16) nat64.push_back({K_NATURAL, k});
    append_matrix(t, 0, off, W, 64, W / 32, nat64, 0, 0); off += (int64_t)W * 64;
    for (int l = 0; l < NH - 1; ++l) { append_matrix(t, 0, off, W, W, W / 32, acc_ksteps(W), 0, 0); off += (int64_t)W * W; }
    append_matrix(t, 0, off, 16, W, 1, acc_ksteps(W), 0, 0); off += 16 * (int64_t)W;
    // mlp_head: [Wh][32] (cols 0..15 SH, 16..30 geo, 31 pad), [Wh][Wh], [16][Wh]
    off = 0;
    append_matrix(t, 1, off, Wh, 32, Wh / 32, {{K_NATURAL, 0}, {K_GEO, 0}}, 16, 31); off += (int64_t)Wh * 32;
    append_matrix(t, 1, off, Wh, Wh, Wh / 32, acc_ksteps(Wh), 0, 0); off += (int64_t)Wh * Wh;
    append_matrix(t, 1, off, 16, Wh, 1, acc_ksteps(Wh), 0, 0);
    // mlp_sem: [Wh][16] (cols 0..14 geo, 15 pad), [Wh][Wh], [sem_pad][Wh]
    off = 0;
    append_matrix(t, 2, off, Wh, 16, Wh / 32, {{K_GEO, 0}}, 0, 15); off += (int64_t)Wh * 16;
    append_matrix(t, 2, off, Wh, Wh, Wh / 32, acc_ksteps(Wh), 0, 0); off += (int64_t)Wh * Wh;
    append_matrix(t, 2, off, sem_pad, Wh, 1, acc_ksteps(Wh), 0, 0);
    return t;
}

int launch_field(mnf_field_t f, const FieldIO &io, bool density_only, hipStream_t stream, const TrainBuf *train) {
    MNF_REQUIRE(f, "field: null handle");
    return f->cfg.mfma_bf16 ? bf16::launch_field_impl(f, io, density_only, stream, train) : f16::launch_field_impl(f, io, density_only, stream, train);
}
}  // namespace mnf

using namespace mnf;

extern "C" int mnf_field_set_params(mnf_field_t f, const float *mlp_base, const float *mlp_head, const float *mlp_sem, mnf_stream_t stream) {
    MNF_REQUIRE(f && mlp_base && mlp_head && mlp_sem, "field_set_params: null argument");
    return f->cfg.mfma_bf16 ? bf16::set_params_impl(f, mlp_base, mlp_head, mlp_sem, false, as_stream(stream))
                            : f16::set_params_impl(f, mlp_base, mlp_head, mlp_sem, false, as_stream(stream));
}

extern "C" int mnf_field_refresh_weights(mnf_field_t f, const float *mlp_base, const float *mlp_head, const float *mlp_sem, mnf_stream_t stream) {
    MNF_REQUIRE(f && mlp_base && mlp_head && mlp_sem, "field_refresh_weights: null argument");
    MNF_REQUIRE(f->params_loaded, "field_refresh_weights: parameters were never loaded (the fp16 table is not current)");
    return f->cfg.mfma_bf16 ? bf16::set_params_impl(f, mlp_base, mlp_head, mlp_sem, true, as_stream(stream))
                            : f16::set_params_impl(f, mlp_base, mlp_head, mlp_sem, true, as_stream(stream));
}

extern "C" void *mnf_field_table_mirror(mnf_field_t f, int64_t *first_param_host) {
    if (!f) return nullptr;
    if (first_param_host) *first_param_host = f->n_base_mlp;
    return f->d_table;
}

extern "C" int mnf_field_create(const mnf_field_config *cfg, mnf_field_t *out) {
    MNF_REQUIRE(cfg && out, "field_create: null argument");
    MNF_REQUIRE(cfg->struct_size == sizeof(mnf_field_config), "field_create: cfg->struct_size is %u, this library's mnf_field_config has %zu bytes (MNF_INIT)",
                cfg->struct_size, sizeof(mnf_field_config));
    MNF_REQUIRE(cfg->neurons == 64 || cfg->neurons == 128, "field_create: neurons must be 64 or 128 (got %d)", cfg->neurons);
    MNF_REQUIRE(cfg->layers >= 1 && cfg->layers <= 4, "field_create: layers must be 1..4 (got %d)", cfg->layers);
    MNF_REQUIRE(cfg->num_semantic_classes >= 1 && cfg->num_semantic_classes <= 32,
                "field_create: num_semantic_classes must be 1..32 (got %d)", cfg->num_semantic_classes);
    MNF_REQUIRE(cfg->n_levels == 16 && cfg->n_features == 4, "field_create: only 16 levels x 4 features are supported");
    MNF_REQUIRE(cfg->log2_hashmap_size >= 8 && cfg->log2_hashmap_size <= 24, "field_create: bad log2_hashmap_size");
    MNF_REQUIRE(!cfg->blend_fp16 || cfg->neurons == 128, "field_create: blend_fp16 is built for neurons = 128 only");
    mnf_field_s *f = new mnf_field_s();
    f->cfg = *cfg;
    grid_levels(*cfg, f->levels, &f->table_entries);
    const int W = cfg->neurons, Wh = W / 2, NH = cfg->layers;
    const int sem_pad = ((cfg->num_semantic_classes + 15) / 16) * 16;
    f->n_base_mlp = (int64_t)W * 64 + (int64_t)(NH - 1) * W * W + 16 * (int64_t)W;
    f->n_base = f->n_base_mlp + f->table_entries * 4;
    f->n_head = (int64_t)Wh * 32 + (int64_t)Wh * Wh + 16 * (int64_t)Wh;
    f->n_sem = (int64_t)Wh * 16 + (int64_t)Wh * Wh + (int64_t)sem_pad * Wh;
    std::vector<int32_t> table = build_frag_table(*cfg);
    f->shape = {W, NH, Wh, cfg->num_semantic_classes, (int)(table.size() / 512)};
    f->frag_src_host = table;
    f->d_table = nullptr; f->d_frags = nullptr; f->d_frag_src = nullptr; f->params_loaded = false; f->d_counter = nullptr;
    f->train_state = nullptr;
    hipError_t e = hipMalloc(&f->d_table, (size_t)f->table_entries * 4 * sizeof(uint16_t) + 64);   // (+ slack: a paired 16-byte gather may start at a level's last entry)
    if (e == hipSuccess) e = hipMalloc(&f->d_frags, table.size() * sizeof(uint16_t) + sizeof(LevelMeta) * 16);
    if (e == hipSuccess) e = hipMalloc((void **)&f->d_frag_src, table.size() * sizeof(int32_t));
    if (e == hipSuccess) e = hipMemcpy(f->d_frag_src, table.data(), table.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy((char *)f->d_frags + table.size() * sizeof(uint16_t), f->levels, sizeof(LevelMeta) * 16, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        set_error("field_create: %s", hipGetErrorString(e));
        mnf_field_destroy(f);
        return MNF_ERR_HIP;
    }
    *out = f;
    return MNF_OK;
}

extern "C" int mnf_field_destroy(mnf_field_t f) {
    if (!f) return MNF_OK;
    free_train_state(f);
    if (f->d_table) (void)hipFree(f->d_table);
    if (f->d_frags) (void)hipFree(f->d_frags);
    if (f->d_frag_src) (void)hipFree(f->d_frag_src);
    if (f->d_counter) (void)hipFree(f->d_counter);
    delete f;
    return MNF_OK;
}

extern "C" int64_t mnf_field_param_count(mnf_field_t f, int32_t which) {
    if (!f) return -1;
    return which == 0 ? f->n_base : (which == 1 ? f->n_head : (which == 2 ? f->n_sem : -1));
}

extern "C" int mnf_field_grid_meta_host(mnf_field_t f, float *scale_host, int32_t *res_host, int32_t *size_host,
                                        int64_t *offset_host, int32_t *hashed_host) {
    MNF_REQUIRE(f, "grid_meta: null handle");
    for (int l = 0; l < f->cfg.n_levels; ++l) {
        if (scale_host) scale_host[l] = f->levels[l].scale;
        if (res_host) res_host[l] = (int32_t)f->levels[l].res;
        if (size_host) size_host[l] = (int32_t)f->levels[l].size;
        if (offset_host) offset_host[l] = (int64_t)f->levels[l].offset;
        if (hashed_host) hashed_host[l] = (int32_t)f->levels[l].hashed;
    }
    return MNF_OK;
}

extern "C" int mnf_field_forward(mnf_field_t f, const float *positions, const float *directions, int64_t n,
                                 float *rgb, float *density, float *sem, mnf_stream_t stream) {
    MNF_REQUIRE(f, "field_forward: null handle");
    MNF_REQUIRE(n >= 0, "field_forward: negative n");
    if (n == 0) return MNF_OK;
    MNF_REQUIRE(positions && directions, "field_forward: null positions/directions");
    FieldIO io = {};
    io.mode = 0; io.positions = positions; io.directions = directions; io.n = n;
    io.rgb = rgb; io.density = density; io.sem = sem;
    return launch_field(f, io, false, as_stream(stream));
}

extern "C" int mnf_field_density(mnf_field_t f, const float *positions, int64_t n, float *density, mnf_stream_t stream) {
    MNF_REQUIRE(f, "field_density: null handle");
    MNF_REQUIRE(n >= 0, "field_density: negative n");
    if (n == 0) return MNF_OK;
    MNF_REQUIRE(positions && density, "field_density: null pointer");
    FieldIO io = {};
    io.mode = 0; io.positions = positions; io.n = n; io.density = density;
    return launch_field(f, io, true, as_stream(stream));
}

extern "C" int mnf_field_forward_samples(mnf_field_t f, const float *rays_o, const float *rays_d, const int64_t *ray_indices,
                                         const float *t_starts, const float *t_ends, int64_t n,
                                         float *rgb, float *density, float *sem, mnf_stream_t stream) {
    MNF_REQUIRE(f, "field_forward_samples: null handle");
    MNF_REQUIRE(n >= 0, "field_forward_samples: negative n");
    if (n == 0) return MNF_OK;
    MNF_REQUIRE(rays_o && rays_d && ray_indices && t_starts && t_ends, "field_forward_samples: null pointer");
    FieldIO io = {};
    io.mode = 1; io.rays_o = rays_o; io.rays_d = rays_d; io.ray_idx64 = ray_indices; io.t_starts = t_starts; io.t_ends = t_ends; io.n = n;
    io.rgb = rgb; io.density = density; io.sem = sem;
    const bool density_only = (rgb == nullptr && sem == nullptr);
    return launch_field(f, io, density_only, as_stream(stream));
}

extern "C" int mnf_field_density_rays(mnf_field_t f, const float *rays_o, const float *rays_d, const int64_t *ray_indices,
                                      const float *t_starts, const float *t_ends, const int64_t *chunk_starts, const int64_t *chunk_cnts,
                                      int32_t n_rays, int64_t n_samples, float early_stop_eps, float *density, mnf_stream_t stream) {
    MNF_REQUIRE(f, "field_density_rays: null handle");
    MNF_REQUIRE(n_rays >= 0 && n_samples >= 0, "field_density_rays: negative size");
    if (n_samples == 0 || n_rays == 0) return MNF_OK;
    MNF_REQUIRE(rays_o && rays_d && ray_indices && t_starts && t_ends && chunk_starts && chunk_cnts && density, "field_density_rays: null pointer");
    hipStream_t s = as_stream(stream);
    if (!f->d_counter) MNF_HIP(hipMalloc((void **)&f->d_counter, 256));
    MNF_HIP(hipMemsetAsync(f->d_counter, 0, sizeof(int32_t), s));
    MNF_HIP(hipMemsetAsync(density, 0, (size_t)n_samples * sizeof(float), s));
    FieldIO io = {};
    io.mode = 3; io.rays_o = rays_o; io.rays_d = rays_d; io.ray_idx64 = ray_indices; io.t_starts = t_starts; io.t_ends = t_ends; io.n = n_samples;
    io.chunk_starts = chunk_starts; io.chunk_cnts = chunk_cnts; io.n_rays = n_rays; io.ray_counter = f->d_counter;
    // skip what lies behind T < eps / 2: the factor 2 keeps the decision clear of the rounding of any other summation order
    io.sdt_stop = early_stop_eps > 0.0f ? -logf(early_stop_eps) + 0.6931472f : INFINITY;
    io.density = density;
    return launch_field(f, io, true, s);
}
