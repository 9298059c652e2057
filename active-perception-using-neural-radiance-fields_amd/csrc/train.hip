// Backward pass of the radiance field (the tiny-cuda-nn backward the reference reaches through
// `loss.backward()`, scripts/pipeline.py:518; forward call sites perception/models/radiance_fields/ngp.py:171-238): the matrix-core half and the
// host code that runs the whole of it (backward_impl).
//
//   dgrad_kernel   dL/d(rgb, sigma, sem) per sample -> pre-activation gradients of every layer (kept in MFMA
//                  registers from layer to layer exactly like the forward chain, with the TRANSPOSED weight
//                  fragments as the A operand), stored feature-major for the weight-gradient GEMMs, and
//                  dL/d(hash features) per sample.
//   wgrad_kernel   dW[n][k] = sum_samples dOut^T[n][c] * In^T[k][c]: the contraction runs over samples, and with
//                  feature-major fp16 activations both MFMA operands are plain 16-byte loads; split over sample
//                  chunks, fp32 atomics into the flat parameter-gradient vectors.
//   scatter.hip    trilinear scatter of dL/d(features) into the dense fp32 table gradient, behind scatter.h.
//
// The optimizer that consumes the gradients is adam.hip.
// Gradients of activations travel in fp16 scaled by `loss_scale` (tcnn does the same with its default scale of
// 128); parameter gradients are accumulated and returned in fp32, un-scaled.
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "field_dev.h"
#include "scatter.h"
#include "workspace.h"

MNF_DT_BEGIN

// ------------------------------------------------------------------ transposed-fragment bookkeeping
template <int W, int NH>
struct LayoutT {
    static constexpr int Wh = W / 2, RT = W / 32, RTh = Wh / 32, KSW = W / 16, KSh = Wh / 16;
    static constexpr int o_r3 = 0;                         // rgb head out^T : RTh x 1
    static constexpr int o_r2 = o_r3 + RTh * 1;            // rgb head hid^T : RTh x KSh
    static constexpr int o_r1 = o_r2 + RTh * KSh;          // rgb head in^T (geo rows) : 1 x KSh
    static constexpr int o_s3 = o_r1 + KSh;                // sem head out^T : RTh x 2
    static constexpr int o_s2 = o_s3 + RTh * 2;
    static constexpr int o_s1 = o_s2 + RTh * KSh;
    static constexpr int o_bo = o_s1 + KSh;                // base out^T : RT x 1
    static constexpr int o_bh = o_bo + RT * 1;             // base hidden^T l : RT x KSW each, l = 0..NH-2
    static constexpr int o_b1 = o_bh + (NH - 1) * RT * KSW;  // base in^T : 2 x KSW
    static constexpr int blocks = o_b1 + 2 * KSW;
};

struct BwdArgs {
    const half8 *fragsT;
    const float *d_rgb, *d_sigma, *d_sem;   // [N,3], [N], [N,C]
    const float *rgb, *sigma;               // forward outputs [N,3], [N]
    float *dX;                              // [16 levels][Np][4] fp32, un-scaled (level-major for hash_bwd)
    int64_t n;
    const int64_t *n_dev;
    int C;
    float loss_scale;
    int chunk, n_chunks;
    TrainBuf train;
    FactoredGrad fg;                        // fg.w != NULL (field.h): d_rgb / d_sem are not read, the products are formed here
};

// fp32 -> fp16 with saturation at the largest finite half: a loss-scaled gradient that leaves the fp16 range is clipped
// instead of becoming Inf (which would poison every weight gradient of the step)
#ifdef MNF_BF16
__device__ __forceinline__ half_t sat_half(float v) { return (half_t)v; }   // bf16 has fp32's range
#else
__device__ __forceinline__ half_t sat_half(float v) { return (half_t)(v != v ? v : fminf(fmaxf(v, -65504.0f), 65504.0f)); }   // NaN stays NaN
#endif

// acc[ct] = sum_ks A(rt, ks) * b[ct][ks] for one 32-row tile
template <int KS>
__device__ __forceinline__ void dense_tile(const half8 *__restrict__ w_lds, int lane, const half8 (&b)[CT][KS], f32x16 (&acc)[CT]) {
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[ct][i] = 0.0f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const half8 a = w_lds[ks * 64 + lane];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) acc[ct] = mfma(a, b[ct][ks], acc[ct]);
    }
}

// One backward layer through a ReLU: dz[ct][2rt+s] = pack(W^T(rt,:) * dOut[ct]) masked by the saved activation,
// stored feature-major at row0 for the weight gradient.
template <int RT_OUT, int KS, int NP>
__device__ __forceinline__ void dense_mask(const half8 *__restrict__ w_lds, int lane, int h, const half8 (&b)[CT][KS],
                                           const u32x4 (&mrec)[NP], int mblock0, const TrainBuf &tb, int64_t tile, int row0,
                                           half_t *stage, half8 (&o)[CT][RT_OUT * 2]) {
#pragma unroll
    for (int rt = 0; rt < RT_OUT; ++rt) {
        f32x16 acc[CT];
        dense_tile<KS>(w_lds + rt * KS * 64, lane, b, acc);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
                // byte (mblock0 + rt * 2 + s) * CT + ct of the lane's mask record (indices are constants once the loops are unrolled)
                const int mb = (mblock0 + rt * 2 + s) * CT + ct;
                const uint32_t m = mrec[mb >> 4][(mb >> 2) & 3] >> (8 * (mb & 3));
                // pack two values per conversion first, then clear the halves whose ReLU was inactive with ONE and: element 2i is
                // bit i of the mask byte, element 2i+1 bit 4+i (frag_mask_bit); a sign-extended 1-bit field extract is an
                // all-ones / all-zeros word.  (Selecting per element before the conversion cost 4.5 instructions per value.)
                u32x4 w;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const half2 p = {(half_t)acc[ct][8 * s + 2 * i], (half_t)acc[ct][8 * s + 2 * i + 1]};
                    const uint32_t lo = (uint32_t)__builtin_amdgcn_sbfe((int)m, i, 1), hi = (uint32_t)__builtin_amdgcn_sbfe((int)m, 4 + i, 1);
                    w[i] = __builtin_bit_cast(uint32_t, p) & ((lo & 0x0000FFFFu) | (hi & 0xFFFF0000u));
                }
                o[ct][rt * 2 + s] = __builtin_bit_cast(half8, w);
            }
            save_pair<true>(tb, tile, row0 + 16 * (rt * 2 + s), lane, stage, o[0][rt * 2 + s], o[1][rt * 2 + s]);
        }
        __builtin_amdgcn_sched_barrier(0);   // keep the row-tile iterations from interleaving (register pressure)
    }
}

template <int W, int NH>
__global__ void __launch_bounds__(kThreads, 2) dgrad_kernel(const BwdArgs args) {
    using L = LayoutT<W, NH>;
    using T = TrainLayout<W, NH>;
    __shared__ half8 s_w[L::blocks * 64];
    __shared__ half_t s_stage[kWavesPerBlock * kStageHalves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, c = lane & 31;
    half_t *stage = s_stage + wave * kStageHalves;
    const int64_t n = count_here(args.n, args.n_dev);
    int64_t tile0, n_tiles;
    chunk_tiles(n, args.chunk, args.n_chunks, tile0, n_tiles);
    if (tile0 + (int64_t)blockIdx.x * kWavesPerBlock >= n_tiles) return;
    for (int i = threadIdx.x; i < L::blocks * 64; i += kThreads) s_w[i] = args.fragsT[i];
    __syncthreads();
    const float ls = args.loss_scale;

    for (int64_t tile = tile0 + (int64_t)blockIdx.x * kWavesPerBlock + wave; tile < n_tiles; tile += (int64_t)gridDim.x * kWavesPerBlock) {
        const int64_t fcol0 = tile * kWaveSamples + c;
        // the lane's ReLU-mask record of the tile: mask_bytes / 16 loads here instead of a byte load per fragment where it is used
        constexpr int kMaskPieces = T::mask_bytes / 16;
        u32x4 mrec[kMaskPieces];
        {
            const u32x4 *mp = reinterpret_cast<const u32x4 *>(args.train.masks + (tile * 64 + lane) * T::mask_bytes);
#pragma unroll
            for (int i = 0; i < kMaskPieces; ++i) mrec[i] = mp[i];
        }
        // ---- output-layer gradients, built directly as natural-order B fragments ----
        half8 dyr[CT][1], dys[CT][2];
        float dlogit[CT];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            const int64_t col = fcol0 + 32 * ct;
            const bool ok = col < n;
#pragma unroll
            for (int j = 0; j < 8; ++j) dyr[ct][0][j] = (half_t)0.0f;
            if (args.fg.w) {      // (wave-uniform) factored output gradients: one weight per sample, the ray's vectors from cache
                const float wv = ok ? args.fg.w[col] : 0.0f;
                const int64_t ry = ok ? args.fg.ray[col] : 0;
                if (ok && h == 0) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const float y = args.rgb[3 * col + k];
                        dyr[ct][0][k] = sat_half(wv * args.fg.g_rgb[3 * ry + k] * y * (1.0f - y) * ls);   // sigmoid'
                    }
                }
#pragma unroll
                for (int s = 0; s < 2; ++s)
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int row = 16 * s + 8 * h + j;
                        dys[ct][s][j] = (ok && row < args.C) ? sat_half(wv * args.fg.g_sem[ry * args.C + row] * ls) : (half_t)0.0f;
                    }
            } else {
            if (ok && h == 0) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const float y = args.rgb[3 * col + k];
                    dyr[ct][0][k] = sat_half(args.d_rgb[3 * col + k] * y * (1.0f - y) * ls);   // sigmoid'
                }
            }
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int row = 16 * s + 8 * h + j;
                    dys[ct][s][j] = (ok && row < args.C) ? sat_half(args.d_sem[col * args.C + row] * ls) : (half_t)0.0f;
                }
            }
            // trunc_exp backward (ngp.py:34-39): g * exp(min(x, 15)) with exp(x) = sigma (0 outside the aabb)
            dlogit[ct] = ok ? args.d_sigma[col] * fminf(args.sigma[col], 3269017.3724721107f) * ls : 0.0f;
        }
        save_pair<false>(args.train, tile, T::rdYr, lane, stage, dyr[0][0], dyr[1][0]);
        save_pair<false>(args.train, tile, T::rdYs, lane, stage, dys[0][0], dys[1][0]);
        save_pair<false>(args.train, tile, T::rdYs + 16, lane, stage, dys[0][1], dys[1][1]);
        // ---- heads ----
        half8 dz2[CT][L::KSh], dz1[CT][L::KSh];
        f32x16 dgeo_r[CT], dgeo_s[CT];
        dense_mask<L::RTh, 1>(s_w + L::o_r3 * 64, lane, h, dyr, mrec, T::mHH2, args.train, tile, T::rdZr2, stage, dz2);
        dense_mask<L::RTh, L::KSh>(s_w + L::o_r2 * 64, lane, h, dz2, mrec, T::mHH1, args.train, tile, T::rdZr1, stage, dz1);
        dense_tile<L::KSh>(s_w + L::o_r1 * 64, lane, dz1, dgeo_r);
        dense_mask<L::RTh, 2>(s_w + L::o_s3 * 64, lane, h, dys, mrec, T::mHS2, args.train, tile, T::rdZs2, stage, dz2);
        dense_mask<L::RTh, L::KSh>(s_w + L::o_s2 * 64, lane, h, dz2, mrec, T::mHS1, args.train, tile, T::rdZs1, stage, dz1);
        dense_tile<L::KSh>(s_w + L::o_s1 * 64, lane, dz1, dgeo_s);
        // ---- base output gradient: geo rows from both heads, row 0 = density logit ----
        half8 dbo[CT][1];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
#pragma unroll
            for (int j = 0; j < 8; ++j) dbo[ct][0][j] = (half_t)(dgeo_r[ct][j] + dgeo_s[ct][j]);
            if (h == 0) dbo[ct][0][0] = sat_half(dlogit[ct]);
        }
        save_pair<true>(args.train, tile, T::rdBO, lane, stage, dbo[0][0], dbo[1][0]);
        // ---- base MLP ----
        half8 dz[CT][L::KSW];
        dense_mask<L::RT, 1>(s_w + L::o_bo * 64, lane, h, dbo, mrec, T::mH0 + (NH - 1) * L::KSW, args.train, tile,
                             T::rdZ0 + (NH - 1) * W, stage, dz);
#pragma unroll
        for (int l = NH - 2; l >= 0; --l) {
            half8 dn[CT][L::KSW];
            dense_mask<L::RT, L::KSW>(s_w + (L::o_bh + l * L::RT * L::KSW) * 64, lane, h, dz, mrec, T::mH0 + l * L::KSW,
                                      args.train, tile, T::rdZ0 + l * W, stage, dn);
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                for (int k = 0; k < L::KSW; ++k) dz[ct][k] = dn[ct][k];
        }
        // ---- gradient of the 64 hash features: rows 32rt + 8g + 4h + i == level (8rt + 2g + h), feature i ----
        const float inv = 1.0f / ls;
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) {
            f32x16 acc[CT];
            dense_tile<L::KSW>(s_w + (L::o_b1 + rt * L::KSW) * 64, lane, dz, acc);
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
                float4 *dst = reinterpret_cast<float4 *>(args.dX) + fcol0 + 32 * ct;   // 32 lanes x 16 B contiguous per level
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    float4 v = {acc[ct][4 * g] * inv, acc[ct][4 * g + 1] * inv, acc[ct][4 * g + 2] * inv, acc[ct][4 * g + 3] * inv};
                    dst[(int64_t)(8 * rt + 2 * g + h) * args.train.Np] = v;
                }
            }
        }
    }
}

// ------------------------------------------------------------------ weight gradients
struct WgradJob {
    int32_t dout_row0, in_row0;   // rows of ACT
    int32_t buf;                  // 0 base, 1 head, 2 sem
    int32_t param_off, stride;    // dW[n][k] lands at param_off + n*stride + colmap[k]
    int32_t n_valid;              // rows of this 32-row tile that exist in the parameter matrix
    int32_t n0;
    int32_t colmap[32];           // parameter column of in-row k of this tile, -1 = none
};

// A group = up to 2 x 2 jobs of one matrix that share their dOut row tiles and their In row tiles.
struct WgradGroup {
    int32_t no, ni;       // dOut tiles and In tiles in the group (1 or 2 each)
    int32_t job[2][2];    // job[o][i]
};

// one wave = one (group, chunk of 64-sample tiles): D[o][i][32][32] += dOut_o^T[32][16 samples] * In_i^T[16 samples][32],
// four MFMA steps per tile and (o, i); the 32 rows of each operand are one contiguous 4 KB block of the tile-major
// activation matrix.  Register blocking 2 x 2 reads each activation row once per two output tiles: the kernel is bound
// by re-reading the activations (44 jobs x 64 rows -> 14 groups, -43 % bytes), not by the MFMAs.
__global__ void __launch_bounds__(256) wgrad_kernel(const WgradJob *__restrict__ jobs, const WgradGroup *__restrict__ groups, int n_groups,
                                                    int split, const half_t *__restrict__ act, int64_t n_cap, const int64_t *n_dev, int rows,
                                                    float inv_scale, float *g0, float *g1, float *g2, float *__restrict__ partials) {
    const int lane = threadIdx.x & 63;
    // a workgroup = four consecutive groups on the SAME range of tiles: groups of one matrix share operand tiles (each dOut / In tile of a hidden matrix is read by
    // two of its four groups), and read by waves of one workgroup at about the same time the second read is a cache hit instead of a second trip to HBM
    const int grp = (blockIdx.x / split) * 4 + (threadIdx.x >> 6);
    const int part = blockIdx.x % split;
    if (grp >= n_groups) return;
    const int wid = grp * split + part;                       // slot of this wave's partial sums (deterministic mode)
    const int64_t n_tiles = (count_here(n_cap, n_dev) + 63) / 64;
    const WgradGroup gp = groups[grp];
    const int64_t t0 = n_tiles * part / split, t1 = n_tiles * (part + 1) / split;
    const int r = lane & 31, h = lane >> 5;
    const bool o2 = gp.no > 1, i2 = gp.ni > 1;   // wave-uniform
    const int dout0 = jobs[gp.job[0][0]].dout_row0, dout1 = o2 ? jobs[gp.job[1][0]].dout_row0 : dout0;
    const int in0 = jobs[gp.job[0][0]].in_row0, in1 = i2 ? jobs[gp.job[0][1]].in_row0 : in0;
    f32x16 acc[2][2];
#pragma unroll
    for (int o = 0; o < 2; ++o)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int k = 0; k < 16; ++k) acc[o][i][k] = 0.0f;
    for (int64_t t = t0; t < t1; ++t) {
        const half_t *base = act + (t * rows + r) * 64 + 8 * h;
        half8 a[2][4], b[2][4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            a[0][q] = *reinterpret_cast<const half8 *>(base + dout0 * 64 + 16 * q);
            b[0][q] = *reinterpret_cast<const half8 *>(base + in0 * 64 + 16 * q);
        }
        if (o2)
#pragma unroll
            for (int q = 0; q < 4; ++q) a[1][q] = *reinterpret_cast<const half8 *>(base + dout1 * 64 + 16 * q);
        if (i2)
#pragma unroll
            for (int q = 0; q < 4; ++q) b[1][q] = *reinterpret_cast<const half8 *>(base + in1 * 64 + 16 * q);
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[0][0] = mfma(a[0][q], b[0][q], acc[0][0]);
        if (i2)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[0][1] = mfma(a[0][q], b[1][q], acc[0][1]);
        if (o2) {
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[1][0] = mfma(a[1][q], b[0][q], acc[1][0]);
            if (i2)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[1][1] = mfma(a[1][q], b[1][q], acc[1][1]);
        }
    }
    if (partials) {   // deterministic mode: this wave's partial sums go to its own slot; wgrad_reduce_kernel adds the slots in a fixed order
        float *dst = partials + ((size_t)wid * 4) * 1024 + lane * 16;
#pragma unroll
        for (int o = 0; o < 2; ++o)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                if (o >= gp.no || i >= gp.ni) continue;
#pragma unroll
                for (int k = 0; k < 16; ++k) dst[(o * 2 + i) * 1024 + k] = acc[o][i][k];
            }
        return;
    }
#pragma unroll
    for (int o = 0; o < 2; ++o)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            if (o >= gp.no || i >= gp.ni) continue;
            const WgradJob &jb = jobs[gp.job[o][i]];
            float *g = jb.buf == 0 ? g0 : (jb.buf == 1 ? g1 : g2);
            const int col = jb.colmap[r];
            if (col < 0) continue;
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int row = (k & 3) + 8 * (k >> 2) + 4 * h;
                if (row < jb.n_valid) atomicAdd(g + jb.param_off + (int64_t)(jb.n0 + row) * jb.stride + col, acc[o][i][k] * inv_scale);
            }
        }
}

// deterministic mode: one thread per element of a (group, o, i) output tile sums the `split` partial slots front to back
__global__ void __launch_bounds__(256) wgrad_reduce_kernel(const WgradJob *__restrict__ jobs, const WgradGroup *__restrict__ groups, int n_groups, int split,
                                                           const float *__restrict__ partials, float inv_scale, float *g0, float *g1, float *g2) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;       // ((group * 4 + oi) * 64 + lane) * 16 + k
    if (e >= (int64_t)n_groups * 4 * 1024) return;
    const int k = (int)(e & 15), lane = (int)((e >> 4) & 63), oi = (int)((e >> 10) & 3), grp = (int)(e >> 12);
    const WgradGroup gp = groups[grp];
    const int o = oi >> 1, i = oi & 1;
    if (o >= gp.no || i >= gp.ni) return;
    const WgradJob &jb = jobs[gp.job[o][i]];
    const int r = lane & 31, h = lane >> 5;
    const int col = jb.colmap[r];
    const int row = (k & 3) + 8 * (k >> 2) + 4 * h;
    if (col < 0 || row >= jb.n_valid) return;
    float sum = 0.0f;
    for (int part = 0; part < split; ++part) sum += partials[(((size_t)grp * split + part) * 4 + oi) * 1024 + lane * 16 + k];
    float *g = jb.buf == 0 ? g0 : (jb.buf == 1 ? g1 : g2);
    g[jb.param_off + (int64_t)(jb.n0 + row) * jb.stride + col] = sum * inv_scale;   // every weight belongs to exactly one tile
}


// ------------------------------------------------------------------ host side: transposed fragments and job table
enum KMapT { T_NATURAL, T_ACC };
enum ColMap { C_IDENT, C_GEO_RGB, C_GEO_SEM };

static int colmap(ColMap m, int i, int n_in_real) {
    if (m == C_IDENT) return i < n_in_real ? i : -1;
    if (i >= 16) return -1;
    if (m == C_GEO_RGB) return i == 0 ? 31 : 15 + i;
    return i == 0 ? 15 : i - 1;
}

// blocks of W^T for one matrix W[n_out][stride]: rows = input features (row_tiles x 32), K = output index n
static void append_matrix_T(std::vector<int32_t> &t, int buf, int64_t off, int n_out_real, int stride, int n_in_real,
                            int row_tiles, ColMap cm, KMapT km, int n_ksteps) {
    for (int rt = 0; rt < row_tiles; ++rt)
        for (int ks = 0; ks < n_ksteps; ++ks)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 8; ++j) {
                    const int r = lane & 31, h = lane >> 5;
                    const int col = colmap(cm, 32 * rt + r, n_in_real);
                    const int n = 16 * ks + (km == T_NATURAL ? 8 * h + j : 8 * (j >> 2) + 4 * h + (j & 3));
                    int32_t v = -1;
                    if (col >= 0 && n < n_out_real) v = (int32_t)((buf << 28) | (int32_t)(off + (int64_t)n * stride + col));
                    t.push_back(v);
                }
}

struct TrainTables {
    std::vector<int32_t> fragT;
    std::vector<WgradJob> jobs;
    std::vector<WgradGroup> groups;
    int rows, mask_blocks, mask_bytes;
    int row_dZr1;      // first row of the rgb head's first-layer pre-activation gradients (the input gradients read them)
};

static void add_jobs(std::vector<WgradJob> &jobs, int buf, int64_t off, int n_out_real, int stride, int n_in_real,
                     int dout_row0, int n_out_tiles, int in_row0, int n_in_tiles, ColMap cm) {
    for (int ot = 0; ot < n_out_tiles; ++ot)
        for (int it = 0; it < n_in_tiles; ++it) {
            WgradJob j;
            j.dout_row0 = dout_row0 + 32 * ot; j.in_row0 = in_row0 + 32 * it; j.buf = buf; j.param_off = (int32_t)off; j.stride = stride;
            j.n0 = 32 * ot;
            j.n_valid = n_out_real - 32 * ot < 32 ? n_out_real - 32 * ot : 32;
            if (j.n_valid < 0) j.n_valid = 0;
            for (int k = 0; k < 32; ++k) j.colmap[k] = colmap(cm, 32 * it + k, n_in_real);
            jobs.push_back(j);
        }
}

// 2 x 2 groups over the (n_out_tiles x n_in_tiles) jobs of one matrix, which add_jobs appended row-major at `first`
static void add_groups(std::vector<WgradGroup> &groups, int first, int n_out_tiles, int n_in_tiles) {
    for (int ot = 0; ot < n_out_tiles; ot += 2)
        for (int it = 0; it < n_in_tiles; it += 2) {
            WgradGroup g;
            g.no = n_out_tiles - ot < 2 ? 1 : 2; g.ni = n_in_tiles - it < 2 ? 1 : 2;
            for (int o = 0; o < 2; ++o)
                for (int i = 0; i < 2; ++i)
                    g.job[o][i] = first + (ot + (o < g.no ? o : 0)) * n_in_tiles + it + (i < g.ni ? i : 0);
            groups.push_back(g);
        }
}

template <int W, int NH>
static TrainTables build_tables(int C) {
    using T = TrainLayout<W, NH>;
    constexpr int Wh = W / 2;
    const int sem_pad = ((C + 15) / 16) * 16;
    TrainTables tt;
    tt.rows = T::rows; tt.mask_blocks = T::mask_blocks; tt.mask_bytes = T::mask_bytes;
    tt.row_dZr1 = T::rdZr1;
    // parameter offsets (reference state_dict layout)
    int64_t b_in = 0, b_hid = (int64_t)W * 64, b_out = b_hid + (int64_t)(NH - 1) * W * W;
    int64_t h_in = 0, h_hid = (int64_t)Wh * 32, h_out = h_hid + (int64_t)Wh * Wh;
    int64_t s_in = 0, s_hid = (int64_t)Wh * 16, s_out = s_hid + (int64_t)Wh * Wh;
    auto &t = tt.fragT;
    append_matrix_T(t, 1, h_out, 16, Wh, Wh, Wh / 32, C_IDENT, T_NATURAL, 1);          // o_r3
    append_matrix_T(t, 1, h_hid, Wh, Wh, Wh, Wh / 32, C_IDENT, T_ACC, Wh / 16);         // o_r2
    append_matrix_T(t, 1, h_in, Wh, 32, 32, 1, C_GEO_RGB, T_ACC, Wh / 16);              // o_r1
    append_matrix_T(t, 2, s_out, sem_pad, Wh, Wh, Wh / 32, C_IDENT, T_NATURAL, 2);     // o_s3
    append_matrix_T(t, 2, s_hid, Wh, Wh, Wh, Wh / 32, C_IDENT, T_ACC, Wh / 16);         // o_s2
    append_matrix_T(t, 2, s_in, Wh, 16, 16, 1, C_GEO_SEM, T_ACC, Wh / 16);              // o_s1
    append_matrix_T(t, 0, b_out, 16, W, W, W / 32, C_IDENT, T_ACC, 1);                  // o_bo
    for (int l = 0; l < NH - 1; ++l) append_matrix_T(t, 0, b_hid + (int64_t)l * W * W, W, W, W, W / 32, C_IDENT, T_ACC, W / 16);   // o_bh
    append_matrix_T(t, 0, b_in, W, 64, 64, 2, C_IDENT, T_ACC, W / 16);                  // o_b1
    // weight-gradient jobs: (dOut rows, In rows), grouped 2 x 2 per matrix
    auto &j = tt.jobs;
    auto matrix = [&](int buf, int64_t off, int n_out_real, int stride, int n_in_real, int dout_row0, int n_out_tiles, int in_row0,
                      int n_in_tiles, ColMap cm) {
        const int first = (int)j.size();
        add_jobs(j, buf, off, n_out_real, stride, n_in_real, dout_row0, n_out_tiles, in_row0, n_in_tiles, cm);
        add_groups(tt.groups, first, n_out_tiles, n_in_tiles);
        return first;
    };
    matrix(0, b_in, W, 64, 64, T::rdZ0, W / 32, T::rX, 2, C_IDENT);
    const size_t hid_g0 = tt.groups.size();
    for (int l = 0; l < NH - 1; ++l)
        matrix(0, b_hid + (int64_t)l * W * W, W, W, W, T::rdZ0 + (l + 1) * W, W / 32, T::rH0 + l * W, W / 32, C_IDENT);
    const size_t hid_g1 = tt.groups.size();
    matrix(0, b_out, 16, W, W, T::rdBO, 1, T::rH0 + (NH - 1) * W, W / 32, C_IDENT);
    // rgb head: in = [SH(16) | geo fragment(16)] (contiguous rows rS..rS+31): SH rows map to columns 0..15
    {
        const int first = matrix(1, h_in, Wh, 32, 32, T::rdZr1, Wh / 32, T::rS, 1, C_IDENT);
        for (size_t q = first; q < j.size(); ++q)
            for (int k = 0; k < 16; ++k) { j[q].colmap[k] = k; j[q].colmap[16 + k] = colmap(C_GEO_RGB, k, 32); }
    }
    matrix(1, h_hid, Wh, Wh, Wh, T::rdZr2, Wh / 32, T::rHH1, Wh / 32, C_IDENT);
    matrix(1, h_out, 16, Wh, Wh, T::rdYr, 1, T::rHH2, Wh / 32, C_IDENT);
    matrix(2, s_in, Wh, 16, 16, T::rdZs1, Wh / 32, T::rG, 1, C_GEO_SEM);
    matrix(2, s_hid, Wh, Wh, Wh, T::rdZs2, Wh / 32, T::rHS1, Wh / 32, C_IDENT);
    matrix(2, s_out, sem_pad, Wh, Wh, T::rdYs, 1, T::rHS2, Wh / 32, C_IDENT);
    // wgrad_kernel runs four consecutive groups in one workgroup on the same tiles: the groups of a hidden matrix (W = 128: 2 x 2 groups that share every operand tile
    // pairwise) go first, so that a set of four is one hidden matrix; behind them base-in (two groups, same In tiles) + base-out (two groups, same dOut tile), then the heads
    std::rotate(tt.groups.begin(), tt.groups.begin() + hid_g0, tt.groups.begin() + hid_g1);
    return tt;
}

// the instantiated shapes (neurons, hidden layers); tools/build_variants.sh builds one
#ifdef MNF_DEV_ONLY_128x2
#define MNF_SHAPES(X) X(128, 2)
#else
#define MNF_SHAPES(X) X(128, 1) X(128, 2) X(128, 3) X(128, 4) X(64, 1) X(64, 2) X(64, 3) X(64, 4)
#endif

static bool tables_for(int W, int NH, int C, TrainTables &tt) {
#define MNF_CASE(w, nh) if (W == w && NH == nh) { tt = build_tables<w, nh>(C); return true; }
    MNF_SHAPES(MNF_CASE)
#undef MNF_CASE
    return false;
}

// Transposed fragments are a re-ordering of the forward fragments the handle already holds in fp16 (every weight sits in
// exactly one forward slot): `src_slot[i]` = forward slot of transposed element i, -1 = structural zero.  No pointer into
// the caller's fp32 vectors is kept between calls.
// Also clears the list cursors of the binned scatter: as a memset at the head of the bins' stream (round 3) the 2.5 KB fill was dispatched
// at the fork, beside the first workgroups of wgrad and the walk, and took 335 us to get through (profiles/r03_train_timeline.txt) — on the
// critical path of the step's tail.  Here it rides on a launch that runs before the fork.
__global__ void __launch_bounds__(256) gather_fragsT_kernel(const int32_t *__restrict__ src_slot, const half_t *__restrict__ frags,
                                                            half_t *__restrict__ dst, int64_t n, uint32_t *__restrict__ cursors, int n_cursors) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_cursors) cursors[i] = 0u;
    if (i >= n) return;
    const int32_t s = src_slot[i];
    dst[i] = s >= 0 ? frags[s] : (half_t)0.0f;
}

struct TrainState {
    TrainTables tt;
    int32_t *d_fragT_src = nullptr;
    half_t *d_fragT = nullptr;
    WgradJob *d_jobs = nullptr;
    WgradGroup *d_groups = nullptr;
    // the hash-table scatter (float atomics, memory-side) runs beside the weight-gradient GEMMs (matrix cores + streaming loads)
    // on a second stream of the handle: both only depend on the backward-data kernel
    hipStream_t side = nullptr;
    hipEvent_t ev_join = nullptr, ev_entry = nullptr;
    hipEvent_t ev_chunk[4] = {nullptr, nullptr, nullptr, nullptr};      // behind each backward-data launch of the chunked pipeline
    // ... and the binned part of the scatter (streams through HBM and LDS) beside the walk (memory-side atomics) on a third
    hipStream_t side2 = nullptr;
    hipEvent_t ev_join2 = nullptr;
    // deterministic mode only (allocated on first use): fixed-point table gradient + replicas, weight-gradient partial slots
    unsigned long long *d_qtable = nullptr;
    float *d_partials = nullptr;
    size_t partials_floats = 0;
    // binned scatter of the large hashed levels (allocated on first use, grows with the sample bound): item lists + list cursors
    uint32_t *d_bin_cursors = nullptr;
    // forward fragment slot of the rgb head's SH weights W1[j][k], j < W/2, k < 16 (the direction gradient stages them from d_frags)
    int32_t *d_sh_slot = nullptr;
};

static int ensure_train_state(mnf_field_t f) {
    if (f->train_state) return MNF_OK;
    TrainState *ts = new TrainState();
    if (!tables_for(f->cfg.neurons, f->cfg.layers, f->cfg.num_semantic_classes, ts->tt)) {
        delete ts;
        set_error("train: unsupported neurons=%d layers=%d", f->cfg.neurons, f->cfg.layers);
        return MNF_ERR_UNSUPPORTED;
    }
    std::vector<int32_t> sh_slot((size_t)(f->cfg.neurons / 2) * 16, -1);
    {   // parameter id -> forward fragment slot
        std::vector<int32_t> slot_of[3];
        slot_of[0].assign((size_t)f->n_base_mlp, -1); slot_of[1].assign((size_t)f->n_head, -1); slot_of[2].assign((size_t)f->n_sem, -1);
        for (size_t i = 0; i < f->frag_src_host.size(); ++i) {
            const int32_t s = f->frag_src_host[i];
            if (s >= 0) slot_of[s >> 28][s & 0x0FFFFFFF] = (int32_t)i;
        }
        for (auto &s : ts->tt.fragT)
            if (s >= 0) s = slot_of[s >> 28][s & 0x0FFFFFFF];
        // rgb head, first layer W1[W/2][32] at offset 0 of the head vector: columns 0..15 are the SH inputs
        for (size_t j = 0; j < sh_slot.size() / 16; ++j)
            for (int k = 0; k < 16; ++k) sh_slot[j * 16 + k] = slot_of[1][j * 32 + k];
    }
    hipError_t e = hipMalloc((void **)&ts->d_fragT_src, ts->tt.fragT.size() * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&ts->d_fragT, ts->tt.fragT.size() * sizeof(uint16_t));
    if (e == hipSuccess) e = hipMalloc((void **)&ts->d_jobs, ts->tt.jobs.size() * sizeof(WgradJob));
    if (e == hipSuccess) e = hipMalloc((void **)&ts->d_groups, ts->tt.groups.size() * sizeof(WgradGroup));
    if (e == hipSuccess) e = hipMemcpy(ts->d_groups, ts->tt.groups.data(), ts->tt.groups.size() * sizeof(WgradGroup), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(ts->d_fragT_src, ts->tt.fragT.data(), ts->tt.fragT.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(ts->d_jobs, ts->tt.jobs.data(), ts->tt.jobs.size() * sizeof(WgradJob), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc((void **)&ts->d_bin_cursors, (size_t)kScatterCursors * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&ts->d_sh_slot, sh_slot.size() * sizeof(int32_t));
    if (e == hipSuccess) e = hipMemcpy(ts->d_sh_slot, sh_slot.data(), sh_slot.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    // side streams: the process-wide ones (common.h shared_side_stream), not a pair per train state
    ts->side = shared_side_stream(0);
    ts->side2 = shared_side_stream(1);
    if (!ts->side || !ts->side2) { delete ts; return MNF_ERR_HIP; }
    for (hipEvent_t *ev : {&ts->ev_join, &ts->ev_entry, &ts->ev_join2, &ts->ev_chunk[0], &ts->ev_chunk[1], &ts->ev_chunk[2], &ts->ev_chunk[3]})
        if (e == hipSuccess) e = hipEventCreateWithFlags(ev, hipEventDisableTiming);
    if (e != hipSuccess) {
        set_error("train: %s", hipGetErrorString(e));
        delete ts;
        return MNF_ERR_HIP;
    }
    f->train_state = ts;
    return MNF_OK;
}

void free_train_state_impl(mnf_field_t f) {
    TrainState *ts = reinterpret_cast<TrainState *>(f->train_state);
    if (!ts) return;
    for (void *p : {(void *)ts->d_fragT_src, (void *)ts->d_fragT, (void *)ts->d_jobs, (void *)ts->d_groups, (void *)ts->d_qtable, (void *)ts->d_partials,
                    (void *)ts->d_bin_cursors, (void *)ts->d_sh_slot})
        if (p) (void)hipFree(p);
    for (hipEvent_t ev : {ts->ev_join, ts->ev_entry, ts->ev_join2, ts->ev_chunk[0], ts->ev_chunk[1], ts->ev_chunk[2], ts->ev_chunk[3]})
        if (ev) (void)hipEventDestroy(ev);
    delete ts;
    f->train_state = nullptr;
}

struct WsView {
    half_t *act; uint8_t *masks; float *dX, *xn, *repl;
    float4 *bin_items;     // item lists of the binned scatter: part of the caller's workspace since round 4 (they were ~720 B per sample of raw
    size_t bin_items_n;    // hipMalloc per train state, invisible to the caller's allocator and grown mid-step)
    int64_t Np, bytes;
};

static WsView carve_train(const TrainTables &tt, const mnf_field_s *f, void *base, int64_t n) {
    WsView v;
    v.Np = ceil_div(n, 64) * 64;
    Carver c(base);
    v.act = c.take<half_t>((size_t)tt.rows * v.Np);
    v.masks = c.take<uint8_t>((size_t)v.Np * tt.mask_bytes);      // [tile][lane] records
    v.dX = c.take<float>((size_t)v.Np * 64);
    v.xn = c.take<float>((size_t)v.Np * 3);
    const ScatterWorkspace sw = scatter_workspace(f, n);
    v.repl = (float *)c.take(sw.repl_bytes);
    v.bin_items_n = sw.bin_items;
    v.bin_items = c.take<float4>(v.bin_items_n);
    v.bytes = c.bytes();
    return v;
}

int64_t train_workspace_bytes_impl(mnf_field_t f, int64_t n) {
    if (!f || n < 0) return -1;
    TrainTables tt;
    if (!tables_for(f->cfg.neurons, f->cfg.layers, f->cfg.num_semantic_classes, tt)) return -1;
    return carve_train(tt, f, nullptr, n).bytes;
}

// The parts of a train workspace the input gradients read (inputgrad.hip), as the last backward on this handle left them.  No HIP call.
int input_grad_view_impl(mnf_field_t f, void *workspace, int64_t n, InputGradView &view) {
    TrainState *ts = reinterpret_cast<TrainState *>(f->train_state);
    MNF_REQUIRE(ts, "field_backward_inputs: no train forward or backward has run on this handle (call mnf_field_backward first)");
    const WsView v = carve_train(ts->tt, f, workspace, n);
    view.act = v.act; view.dX = v.dX; view.xn = v.xn; view.Np = v.Np;
    view.rows = ts->tt.rows; view.row_dZr1 = ts->tt.row_dZr1; view.sh_slot = ts->d_sh_slot;
    return MNF_OK;
}

// the handle's train state (built on first use) and the caller's workspace carved for n samples
static int open_train(mnf_field_t f, const char *who, void *workspace, int64_t workspace_bytes, int64_t n, TrainState *&ts, WsView &v) {
    if (const int rc = ensure_train_state(f)) return rc;
    ts = reinterpret_cast<TrainState *>(f->train_state);
    v = carve_train(ts->tt, f, workspace, n);
    return check_workspace(who, workspace, workspace_bytes, v.bytes);
}

int forward_train_impl(mnf_field_t f, const FieldIO &io, void *workspace, int64_t workspace_bytes, hipStream_t stream, bool deterministic) {
    MNF_REQUIRE(f && f->params_loaded, "field_forward_train: parameters not loaded");
    MNF_REQUIRE(io.n >= 0, "field_forward_train: negative n");
    if (io.n == 0) return MNF_OK;
    TrainState *ts = nullptr;
    WsView v;
    if (const int rc = open_train(f, "field_forward_train", workspace, workspace_bytes, io.n, ts, v)) return rc;
    TrainBuf tb = {v.act, v.masks, v.Np, ts->tt.rows};
    return launch_field_impl(f, io, false, stream, &tb);
}

// ------------------------------------------------------------------ the backward, stage by stage (backward_impl runs them top to bottom)
// no parameter gradients (the fused train render with frozen parameters, mnf_train_render_backward_rays): the output gradients and dgrad run as ever and leave dX
// and the activation gradients in the workspace; no weight gradients, no hash scatter, no side stream
static bool is_frozen(const BackwardCall &c) { return !c.g_base && !c.g_head && !c.g_sem; }

static int bwd_check_and_zero(mnf_field_t f, const BackwardCall &c) {
    MNF_REQUIRE(f && f->params_loaded, "field_backward: parameters not loaded");
    MNF_REQUIRE(c.n >= 0 && c.loss_scale > 0.f, "field_backward: bad arguments");
    const bool frozen = is_frozen(c);
    MNF_REQUIRE(frozen || (c.g_base && c.g_head && c.g_sem), "field_backward: null gradient buffer");
    if (c.zero_grads && !frozen) {
        MNF_HIP(hipMemsetAsync(c.g_base, 0, (size_t)f->n_base * 4, c.stream));
        MNF_HIP(hipMemsetAsync(c.g_head, 0, (size_t)f->n_head * 4, c.stream));
        MNF_HIP(hipMemsetAsync(c.g_sem, 0, (size_t)f->n_sem * 4, c.stream));
    }
    MNF_REQUIRE(c.n == 0 || (c.positions && c.d_density && c.rgb && c.density && (c.factored.w || (c.d_rgb && c.d_sem))), "field_backward: null pointer");
    return MNF_OK;
}

// The scatter's replica buffers are zeroed on the side stream while the backward-data kernel runs (behind the caller's earlier work:
// the workspace may have served another call on this stream a moment ago), not between that kernel and the scatter.
static int bwd_fork(mnf_field_t f, const BackwardCall &c, TrainState *ts, const WsView &v) {
    MNF_HIP(hipEventRecord(ts->ev_entry, c.stream));
    MNF_HIP(hipStreamWaitEvent(ts->side, ts->ev_entry, 0));
    return scatter_begin(f, v.repl, c.deterministic, ts->side);
}

// Chunked pipeline (float-atomic mode, large batches): the backward-data kernel is launched for contiguous ranges of tiles and the scatter of a
// range (walk on the side stream, pass A of the bins on the third) starts behind ITS launch, beside the next range's dgrad: dgrad writes activations
// through the matrix cores and HBM stores, the scatter is bound by the memory-side atomic unit — the two overlap, and only the last range's scatter
// (and the weight gradients, which read every range) is left behind the last dgrad.  One range = the old schedule (deterministic mode: its grouping
// of partial sums must not change).
static int dgrad_ranges(const BackwardCall &c) {
    static const int chunks_env = diag_env("MNF_BWD_CHUNKS") ? atoi(diag_env("MNF_BWD_CHUNKS")) : 0;
    if (c.deterministic || is_frozen(c)) return 1;      // (the ranges exist to start a scatter early: without one, one launch)
    if (chunks_env >= 1 && chunks_env <= 4) return chunks_env;
    return c.n >= ((int64_t)1 << 18) ? 2 : 1;           // measured (profiles/r04_bwd_chunks.txt): 5.77 / 5.52 / 5.60 ms per step with 1 / 2 / 4 ranges.
}

// gather_fragsT (which also clears the scatter's list cursors, in front of the fork points), the normalised positions, then dgrad range by range with
// ev_chunk[k] recorded behind range k: its scatter may start (the weight gradients stay on the caller's stream)
static int bwd_dgrad(mnf_field_t f, const BackwardCall &c, TrainState *ts, const WsView &v, int n_chunks) {
    hipStream_t s = c.stream;
    const int64_t n = c.n;
    // transposed fp16 weight fragments from the handle's forward fragments (the parameters of the last set_params)
    const int64_t n_frag = (int64_t)ts->tt.fragT.size();
    hipLaunchKernelGGL(gather_fragsT_kernel, dim3((unsigned)ceil_div(n_frag > kScatterCursors ? n_frag : (int64_t)kScatterCursors, 256)), dim3(256), 0, s, ts->d_fragT_src,
                       reinterpret_cast<const half_t *>(f->d_frags), ts->d_fragT, n_frag, ts->d_bin_cursors, kScatterCursors);
    BwdArgs a;
    a.fg = c.factored;
    a.fragsT = reinterpret_cast<const half8 *>(ts->d_fragT);
    a.d_rgb = c.d_rgb; a.d_sigma = c.d_density; a.d_sem = c.d_sem; a.rgb = c.rgb; a.sigma = c.density;
    a.dX = v.dX; a.n = n; a.n_dev = c.n_dev; a.C = f->cfg.num_semantic_classes; a.loss_scale = c.loss_scale;
    a.train = {v.act, v.masks, v.Np, ts->tt.rows};
    if (!c.positions_normalized) scatter_normalize(f, c.positions, n, c.n_dev, v.xn, s);   // (the train step's forward hands over normalised positions already: FieldIO::xn_out)
    const int64_t chunk_tiles_max = ceil_div(ceil_div(n, kWaveSamples), n_chunks) + 1;      // tiles of one range, at most
    const int grid = (int)std::min<int64_t>(256, ceil_div(chunk_tiles_max, kWavesPerBlock));
    const int W = f->cfg.neurons, NH = f->cfg.layers;
    const bool frozen = is_frozen(c);
    bool ok = false;
    const int prof_dgrad = prof_start("dgrad", s);
    for (int k = 0; k < n_chunks; ++k) {
        a.chunk = k; a.n_chunks = n_chunks;
#define MNF_CASE(w, nh) if (W == w && NH == nh) { hipLaunchKernelGGL((dgrad_kernel<w, nh>), dim3(grid), dim3(kThreads), 0, s, a); ok = true; }
        MNF_SHAPES(MNF_CASE)
#undef MNF_CASE
        if (!frozen) MNF_HIP(hipEventRecord(ts->ev_chunk[k], s));
    }
    prof_stop(prof_dgrad, s);
    MNF_REQUIRE(ok, "field_backward: unsupported shape");
    return launch_status("dgrad_kernel");
}

static int bwd_wgrad(const BackwardCall &c, TrainState *ts, const WsView &v) {
    hipStream_t s = c.stream;
    const bool deterministic = c.deterministic;
    const int n_groups = (int)ts->tt.groups.size();
    // enough sample chunks to fill the chip with waves (the loop is load-latency bound; 2 x 2 blocking leaves room for
    // ~3 waves per SIMD), but at least 16 tiles per wave so the final atomics stay negligible (sized on the upper bound `n`)
    const int64_t n_tiles = v.Np / 64;
    // (12 waves per CU and 14 groups: 219 tile ranges; the deterministic mode's grouping of partial sums depends on this value and keeps it.  With float atomics
    //  18 per CU — 329 ranges — is 20-40 us ahead at 1.0 M samples: 3.211 / 3.184 / 3.187 / 3.104 ms per step with 219 / 330 / 440 / 660, MNF_WGRAD_SPLIT)
    int split = (int)(256 * (deterministic ? 12 : 18) / n_groups);
    if (!deterministic) {
        static const int split_env = diag_env("MNF_WGRAD_SPLIT") ? atoi(diag_env("MNF_WGRAD_SPLIT")) : 0;
        if (split_env > 0) split = split_env;
    }
    if (split > n_tiles / 16) split = (int)(n_tiles / 16);
    if (split < 1) split = 1;
    float *partials = nullptr;
    if (deterministic) {
        const size_t need = (size_t)n_groups * split * 4 * 1024;
        if (ts->partials_floats < need) {
            if (ts->d_partials) (void)hipFree(ts->d_partials);
            ts->d_partials = nullptr; ts->partials_floats = 0;
            MNF_HIP(hipMalloc((void **)&ts->d_partials, need * sizeof(float)));
            ts->partials_floats = need;
        }
        partials = ts->d_partials;
    }
    static const bool no_wgrad = diag_env("MNF_NO_WGRAD") != nullptr;    // timing experiments: the scatter alone on the chip
    if (!no_wgrad) {
        ProfScope ps("wgrad", s);
        hipLaunchKernelGGL(wgrad_kernel, dim3((unsigned)(ceil_div(n_groups, 4) * split)), dim3(256), 0, s, ts->d_jobs, ts->d_groups, n_groups,
                           split, v.act, c.n, c.n_dev, ts->tt.rows, 1.0f / c.loss_scale, c.g_base, c.g_head, c.g_sem, partials);
        if (partials)
            hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)ceil_div((int64_t)n_groups * 4 * 1024, 256)), dim3(256), 0, s, ts->d_jobs, ts->d_groups,
                               n_groups, split, (const float *)partials, 1.0f / c.loss_scale, c.g_base, c.g_head, c.g_sem);
    }
    return launch_status("wgrad_kernel");
}

// hash-table gradient (side streams): the walk on `side`, the bins on `side2`
static int bwd_scatter(mnf_field_t f, const BackwardCall &c, TrainState *ts, const WsView &v, int n_chunks) {
    const ScatterCall sc = {f, v.dX, c.positions_normalized ? c.positions : v.xn, v.Np, c.n, c.n_dev, c.g_base + f->n_base_mlp, v.repl, v.bin_items, v.bin_items_n,
                            n_chunks, c.deterministic, c.stream, ts->side, ts->side2, ts->ev_chunk, ts->ev_join2, &ts->d_qtable, ts->d_bin_cursors};
    return scatter_run(sc);
}

int backward_impl(mnf_field_t f, const BackwardCall &c) {
    int rc = bwd_check_and_zero(f, c);
    if (rc || c.n == 0) return rc;
    TrainState *ts = nullptr;
    WsView v;
    if ((rc = open_train(f, "field_backward", c.workspace, c.workspace_bytes, c.n, ts, v))) return rc;      // carve
    const bool frozen = is_frozen(c);
    if (!frozen && (rc = bwd_fork(f, c, ts, v))) return rc;
    const int n_chunks = dgrad_ranges(c);
    if ((rc = bwd_dgrad(f, c, ts, v, n_chunks)) || frozen) return rc;
    if ((rc = bwd_wgrad(c, ts, v))) return rc;
    if ((rc = bwd_scatter(f, c, ts, v, n_chunks))) return rc;
    // ---- join
    MNF_HIP(hipEventRecord(ts->ev_join, ts->side));
    MNF_HIP(hipStreamWaitEvent(c.stream, ts->ev_join, 0));
    return rc;
}

MNF_DT_END

#ifndef MNF_BF16   // ---- operand-type independent: compiled once
// fn of the handle's operand type
#define MNF_BY_TYPE(f, fn, ...) ((f)->cfg.mfma_bf16 ? bf16::fn(__VA_ARGS__) : f16::fn(__VA_ARGS__))
namespace mnf {
void free_train_state(mnf_field_t f) { MNF_BY_TYPE(f, free_train_state_impl, f); }
int forward_train(mnf_field_t f, const FieldIO &io, void *workspace, int64_t workspace_bytes, hipStream_t stream, bool deterministic) {
    MNF_REQUIRE(f, "field_forward_train: null handle");
    return MNF_BY_TYPE(f, forward_train_impl, f, io, workspace, workspace_bytes, stream, deterministic);
}
int backward(mnf_field_t f, const BackwardCall &c) {
    MNF_REQUIRE(f, "field_backward: null handle");
    return MNF_BY_TYPE(f, backward_impl, f, c);
}
}  // namespace mnf

using namespace mnf;

extern "C" int64_t mnf_field_train_workspace_bytes(mnf_field_t f, int64_t n) {
    if (!f) return -1;
    return MNF_BY_TYPE(f, train_workspace_bytes_impl, f, n);
}

extern "C" int mnf_field_forward_train(mnf_field_t f, const float *positions, const float *directions, int64_t n,
                                       float *rgb, float *density, float *sem, void *workspace, int64_t workspace_bytes,
                                       mnf_stream_t stream) {
    MNF_REQUIRE(f, "field_forward_train: null handle");
    MNF_REQUIRE(n == 0 || (positions && directions && rgb && density && sem), "field_forward_train: null pointer");
    FieldIO io = {};
    io.mode = 0; io.positions = positions; io.directions = directions; io.n = n;
    io.rgb = rgb; io.density = density; io.sem = sem;
    return MNF_BY_TYPE(f, forward_train_impl, f, io, workspace, workspace_bytes, as_stream(stream), false);
}

extern "C" int mnf_field_forward_train_samples(mnf_field_t f, const float *rays_o, const float *rays_d, const int64_t *ray_indices,
                                               const float *t_starts, const float *t_ends, int64_t n, float *rgb, float *density,
                                               float *sem, float *positions_out, void *workspace, int64_t workspace_bytes,
                                               mnf_stream_t stream) {
    MNF_REQUIRE(f, "field_forward_train_samples: null handle");
    MNF_REQUIRE(n == 0 || (rays_o && rays_d && ray_indices && t_starts && t_ends && rgb && density && sem && positions_out),
                "field_forward_train_samples: null pointer");
    FieldIO io = {};
    io.mode = 1; io.rays_o = rays_o; io.rays_d = rays_d; io.ray_idx64 = ray_indices; io.t_starts = t_starts; io.t_ends = t_ends; io.n = n;
    io.rgb = rgb; io.density = density; io.sem = sem; io.positions_out = positions_out;
    return MNF_BY_TYPE(f, forward_train_impl, f, io, workspace, workspace_bytes, as_stream(stream), false);
}

extern "C" int mnf_field_backward(mnf_field_t f, const float *positions, int64_t n,
                                  const float *d_rgb, const float *d_density, const float *d_sem,
                                  const float *rgb, const float *density,
                                  void *workspace, int64_t workspace_bytes, float loss_scale,
                                  float *g_base, float *g_head, float *g_sem, mnf_stream_t stream) {
    MNF_REQUIRE(f, "field_backward: null handle");
    MNF_REQUIRE(g_base && g_head && g_sem, "field_backward: null gradient buffer");
    BackwardCall c = {};
    c.positions = positions; c.n = n; c.d_rgb = d_rgb; c.d_density = d_density; c.d_sem = d_sem; c.rgb = rgb; c.density = density; c.workspace = workspace;
    c.workspace_bytes = workspace_bytes; c.loss_scale = loss_scale; c.g_base = g_base; c.g_head = g_head; c.g_sem = g_sem; c.zero_grads = true; c.stream = as_stream(stream);
    return backward(f, c);
}

#endif  // MNF_BF16
