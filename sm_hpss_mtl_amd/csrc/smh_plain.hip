// The four feature branches of get_featuregram WITHOUT the harmonic-percussive separation (lib/preprocessing.py:378-402):
//
//   Spec        fv = |S|                                   (:380)          rows = K
//   LogSpec     fv = power_to_db(|S|**2)                   (:384-385)      rows = K
//   MelSpec     fv = melspectrogram(y=Xin, sr=fs, ...)     (:394)          rows = n_mels     = mel(sr = fs) @ |S|**2
//   LogMelSpec  fv = power_to_db(melspectrogram(y=...)**2) (:400-401)      rows = n_mels
//
// Two things differ from the '*HarmPerc*' branches and are fixed HERE, not left to a composition of stage calls: the mel branches
// project the POWER spectrogram (melspectrogram(y=...) takes librosa's default power = 2.0), and their basis is built for sr = fs
// (the context's mel_sr; the host layer sets it to fs for these names).  The squares are f32 products, as numpy's.
//
// Two kernels behind the unchanged STFT, both over a clip table (smh_rag::Clip) or, without one, over B equal clips:
//
//   plain_project_kernel   one workgroup per (clip, 64-frame tile), 8 waves.  A row of S is read by one wave as 64 consecutive
//       floats (256 bytes); the K x 64 image goes to LDS squared (mel) and the CSR filters are applied from there, a wave per filter
//       row, a lane per frame: conflict-free LDS reads at stride 1, the filter's taps wave-uniform.  fv rows leave as 256-byte
//       stores.  Without a filterbank the image passes through registers.  Log features: the un-squared value x is stored and the
//       clip's maximum goes wave reduction -> LDS -> ONE atomicMax per workgroup on the int key (x >= 0: floats order like their
//       bits), one key per clip.
//   plain_finish_kernel    one workgroup per (clip, block of 32 rows), 4 waves of 8 rows.  Pass 1: the rows' StandardScaler
//       statistics in float64 over the final dB values (formed on the fly), lanes striding the row by 64 and an xor-shuffle tree: the
//       summation order depends on T alone.  Pass 2, per 64-frame chunk: dB + the max - 80 floor -> the final fv (in place); the
//       standardised values go to a [32][65] LDS tile and leave it transposed, as 128-byte runs of 32 rows in every patch that
//       holds the frame (tools.extract_patches' grid on the tiled-if-short featuregram, time-major).  IMAGE instantiation: the
//       Conv2D models' layout (nP, rows, W) instead.  A lane holds one frame of a row, and consecutive frames of a row are
//       consecutive floats of a patch row, so the same values leave straight from the registers as runs of up to 256 bytes along
//       the patch's time axis: no LDS tile, no barrier.
//
// Tiles and row blocks are independent, so every T >= 1 takes this one route, alone, in an equal-length batch or in a ragged one,
// and gets the same bits in each.
#include <algorithm>
#include <cstring>
#include <vector>

#include "smh_common.h"
#include "smh_feat.h"
#include "smh_rag.h"

namespace {

using smh_feat::final_value;
using smh_feat::floor_of_max;
using smh_feat::MelTable;
using smh_feat::PatchOut;
using smh::xcd_item;
using smh_rag::align_up;
using smh_rag::Clip;
using smh_rag::HostClip;
using smh_rag::Item;
using smh_rag::Layout;

constexpr int kTile = 64;        // frames per projection workgroup and per finishing chunk: one lane per frame
constexpr int kProjWaves = 8;
constexpr int kRowBlock = 32;    // rows per finishing workgroup: 128-byte runs in the time-major patches
constexpr int kFinWaves = 4;
constexpr int kRowsPerWave = kRowBlock / kFinWaves;
constexpr size_t kMaxImageBytes = 150 * 1024;

// the clips of a launch: a descriptor table (ragged calls) or, with clips == nullptr, B equal clips of T frames laid out densely
struct Geo {
    const Clip *clips;
    const Item *items;  // projection work list (clip, tile) of a ragged call
    int n_items;        // projection workgroups
    int T, Ttiled, nP, ntiles;  // the equal-length shape
};

struct ClipView {
    size_t spec_off, fv_off, patch_off;  // floats into S / fv, patches in front of this clip's
    int T, Ttiled, nP;
};

__device__ __forceinline__ ClipView clip_view(const Geo &g, int K, int rows, int clip) {
    ClipView v;
    if (g.clips) {
        const Clip &c = g.clips[clip];
        v.spec_off = (size_t)c.spec_off, v.fv_off = (size_t)c.fv_off, v.patch_off = (size_t)c.patch_off;
        v.T = c.T, v.Ttiled = c.Ttiled, v.nP = c.nP;
    } else {
        v.spec_off = (size_t)clip * K * g.T, v.fv_off = (size_t)clip * rows * g.T, v.patch_off = (size_t)clip * g.nP;
        v.T = g.T, v.Ttiled = g.Ttiled, v.nP = g.nP;
    }
    return v;
}

__global__ void __launch_bounds__(64 * kProjWaves)
plain_project_kernel(MelTable mt, const float *__restrict__ S, int K, int rows, int want_max, float *__restrict__ fv,
                     int *__restrict__ maxkeys, Geo g) {
    extern __shared__ __attribute__((aligned(16))) float img[];  // [K][kTile], mel contexts only
    __shared__ int wkey[kProjWaves];
    unsigned n;
    if (!xcd_item(g.n_items, n)) return;
    int clip, tile;
    if (g.items) {
        const Item it = g.items[n];
        clip = it.clip, tile = it.tile;
    } else {
        clip = (int)(n / (unsigned)g.ntiles), tile = (int)(n - (unsigned)clip * (unsigned)g.ntiles);
    }
    const ClipView c = clip_view(g, K, rows, clip);
    const int T = c.T, t0 = tile * kTile;
    const int nt = min(kTile, T - t0);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    // lanes beyond the clip's last frame read that frame again: their values change no maximum and are never stored
    const float *Sc = S + c.spec_off + t0 + min(lane, nt - 1);
    float *out = fv + c.fv_off + t0 + lane;
    const bool live = lane < nt;
    float mx = 0.f;  // every value is a magnitude, a square or a sum of non-negative products
    constexpr int kB = 4;  // rows of loads in flight per wave
    if (mt.n_mels <= 0) {
        for (int k0 = wave; k0 < K; k0 += kProjWaves * kB) {
            float v[kB];
#pragma unroll
            for (int q = 0; q < kB; ++q) v[q] = Sc[(size_t)min(k0 + q * kProjWaves, K - 1) * T];
#pragma unroll
            for (int q = 0; q < kB; ++q) {
                const int k = k0 + q * kProjWaves;
                if (k < K) {
                    if (live) out[(size_t)k * T] = v[q];
                    mx = fmaxf(mx, v[q]);
                }
            }
        }
    } else {
        for (int k0 = wave; k0 < K; k0 += kProjWaves * kB) {
            float v[kB];
#pragma unroll
            for (int q = 0; q < kB; ++q) v[q] = Sc[(size_t)min(k0 + q * kProjWaves, K - 1) * T];
#pragma unroll
            for (int q = 0; q < kB; ++q) {
                const int k = k0 + q * kProjWaves;
                if (k < K) img[k * kTile + lane] = v[q] * v[q];  // |S|**2 in f32 (melspectrogram's power = 2.0)
            }
        }
        __syncthreads();
        for (int m = wave; m < mt.n_mels; m += kProjWaves) {
            const int start = mt.start[m], cnt = mt.count[m];  // wave-uniform: start + cnt <= K
            const float *w = mt.w + mt.off[m];
            const float *col = img + start * kTile + lane;
            float acc = 0.f;
            for (int j = 0; j < cnt; ++j) acc = fmaf(w[j], col[j * kTile], acc);
            if (live) out[(size_t)m * T] = acc;
            mx = fmaxf(mx, acc);
        }
    }
    if (!want_max) return;
    int key = __float_as_int(mx);
    for (int off = 32; off > 0; off >>= 1) key = max(key, __shfl_xor(key, off));
    if (lane == 0) wkey[wave] = key;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 1; i < kProjWaves; ++i) key = max(key, wkey[i]);
        atomicMax(&maxkeys[clip], key);
    }
}

template <bool IMAGE>
__global__ void __launch_bounds__(64 * kFinWaves)
plain_finish_kernel(float *__restrict__ fv, const int *__restrict__ maxkeys, int log_db, int K, int rows, int nrb, int W, int shift,
                    float *__restrict__ patches, Geo g) {
    float *tile = nullptr;  // the transposing LDS tile: time-major only
    if constexpr (!IMAGE) {
        __shared__ float tile_lds[kRowBlock * (kTile + 1)];
        tile = tile_lds;
    }
    const int clip = blockIdx.x / nrb, rb = blockIdx.x - clip * nrb;
    const ClipView c = clip_view(g, K, rows, clip);
    const int T = c.T;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int r0 = rb * kRowBlock, nr = min(kRowBlock, rows - r0);
    const float lim = log_db ? floor_of_max(maxkeys[clip]) : 0.f;
    const bool want = patches != nullptr && c.nP > 0;
    float *x[kRowsPerWave];  // this wave's rows: r0 + 4 q + wave; rows beyond the block repeat its last one and are never written
#pragma unroll
    for (int q = 0; q < kRowsPerWave; ++q) x[q] = fv + c.fv_off + (size_t)(r0 + min(q * kFinWaves + wave, nr - 1)) * T;
    double mean[kRowsPerWave];
    float inv[kRowsPerWave];
    if (want) {
        // StandardScaler per row over the frames (lib/preprocessing.py:211-214), float64, one pass over d = value - the row's first
        // value.  The tiled-if-short featuregram repeats the row, which changes neither its mean nor its population variance; the
        // constant-row rule (sklearn's _is_constant_feature) counts the tiled frames.
        double x0[kRowsPerWave], s[kRowsPerWave], sq[kRowsPerWave];
#pragma unroll
        for (int q = 0; q < kRowsPerWave; ++q) x0[q] = (double)final_value(x[q][0], lim, log_db), s[q] = 0.0, sq[q] = 0.0;
        for (int t = lane; t < T; t += 64) {
            float v[kRowsPerWave];
#pragma unroll
            for (int q = 0; q < kRowsPerWave; ++q) v[q] = x[q][t];
#pragma unroll
            for (int q = 0; q < kRowsPerWave; ++q) {
                const double d = (double)final_value(v[q], lim, log_db) - x0[q];
                s[q] += d;
                sq[q] += d * d;
            }
        }
#pragma unroll
        for (int q = 0; q < kRowsPerWave; ++q) {
            double a = s[q], b = sq[q];
            for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off), b += __shfl_xor(b, off);
            double inv_scale;
            smh_feat::scaler_of_sums(x0[q], a, b, T, c.Ttiled, mean[q], inv_scale);
            inv[q] = (float)inv_scale;
        }
    }
    if (!want && !log_db) return;  // nothing to finish: fv is final as projected
    const int f = threadIdx.x & (kRowBlock - 1), tl0 = threadIdx.x >> 5;
    for (int c0 = 0; c0 < T; c0 += kTile) {
        const int nt = min(kTile, T - c0);
        const int tc = c0 + min(lane, nt - 1);
        float v[kRowsPerWave];
#pragma unroll
        for (int q = 0; q < kRowsPerWave; ++q) v[q] = x[q][tc];
#pragma unroll
        for (int q = 0; q < kRowsPerWave; ++q) {
            const int rl = q * kFinWaves + wave;
            if (rl < nr) {
                const float d = final_value(v[q], lim, log_db);
                if (log_db && lane < nt) x[q][c0 + lane] = d;  // the FINAL featuregram
                // (x - mean) rounded to f32 as sklearn does, then * 1 / scale
                if (want) {
                    const float z = (float)((double)d - mean[q]) * inv[q];
                    if constexpr (IMAGE) v[q] = z;
                    else tile[rl * (kTile + 1) + lane] = z;
                }
            }
        }
        if (!want) continue;
        if constexpr (IMAGE) {
            for (int u = lane < nt ? c0 + lane : c.Ttiled; u < c.Ttiled; u += T) {  // the frame's positions in the tiled featuregram (one unless T < W)
                int p_lo, p_hi;
                smh_feat::patch_range(u, W, shift, c.nP, p_lo, p_hi);
                for (int p = p_lo; p <= p_hi; ++p) {
                    float *dst = patches + ((c.patch_off + (size_t)p) * rows + r0 + wave) * W + (u - p * shift);
#pragma unroll
                    for (int q = 0; q < kRowsPerWave; ++q)
                        if (q * kFinWaves + wave < nr) dst[(size_t)q * kFinWaves * W] = v[q];
                }
            }
        } else {
            __syncthreads();
            const int nP = c.nP, Tt = c.Ttiled;
            for (int tl = tl0; tl < nt; tl += (64 * kFinWaves) / kRowBlock) {
                for (int u = c0 + tl; u < Tt; u += T) {  // the frame's positions in the tiled featuregram (one unless T < W)
                    int p_lo, p_hi;
                    smh_feat::patch_range(u, W, shift, nP, p_lo, p_hi);
                    for (int p = p_lo; p <= p_hi; ++p) {
                        const int j = u - p * shift;
                        if (f < nr) patches[((c.patch_off + (size_t)p) * W + j) * rows + r0 + f] = tile[f * (kTile + 1) + tl];
                    }
                }
            }
            __syncthreads();
        }
    }
}

// both kernels over n_clips clips described by g; keys: n_clips ints, zero on entry when the context is a log one
int launch_pair(const smh_ctx *ctx, const float *S, float *fv, const PatchOut &po, int *keys, const Geo &g, int n_clips, hipStream_t st) {
    const int K = ctx->K, rows = ctx->feat_rows, log_db = ctx->cfg.log_db ? 1 : 0;
    if (n_clips <= 0 || g.n_items <= 0) return SMH_OK;
    const size_t lds = ctx->n_mels > 0 ? sizeof(float) * (size_t)K * kTile : 0;
    const unsigned gp = smh::xcd_grid(g.n_items);
    // (the attribute never below 1024: a spectrogram context launches with no dynamic LDS at all)
    int rc = smh::launch_lds(plain_project_kernel, "plain_project_kernel", dim3(gp), dim3(64 * kProjWaves), lds, std::max<size_t>(lds, 1024), st,
                             smh_feat::mel_table(ctx), S, K, rows, log_db, fv, keys, g);
    if (rc) return rc;
    if (!log_db && !po.patches) return SMH_OK;
    const int nrb = (rows + kRowBlock - 1) / kRowBlock;
    const auto finish = po.layout == smh_feat::kLayoutImage && po.patches ? plain_finish_kernel<true> : plain_finish_kernel<false>;
    hipLaunchKernelGGL(finish, dim3((unsigned)n_clips * (unsigned)nrb), dim3(64 * kFinWaves), 0, st, fv, (const int *)keys,
                       log_db, K, rows, nrb, po.W, po.shift, po.patches, g);
    return smh::launch_status("plain_finish_kernel");
}

int check_context(const smh_ctx *ctx, const char *who) {
    SMH_REQUIRE(ctx->n_mels <= 0 || sizeof(float) * (size_t)ctx->K * kTile <= kMaxImageBytes,
                "%s: n_fft=%d is too large for the %d-frame LDS image of the mel projection", who, ctx->cfg.n_fft, kTile);
    return SMH_OK;
}

inline bool layout_ok(int patch_layout) { return patch_layout == smh_feat::kLayoutImage || patch_layout == smh_feat::kLayoutTimeMajor; }

}  // namespace

extern "C" int smh_plain_features_f32(const smh_ctx *ctx, const float *d_S, int B, int T, int W, int shift, float *d_fv,
                                      float *d_patches, int32_t *d_maxkeys, void *stream) {
    return smh_plain_features_layout_f32(ctx, d_S, B, T, W, shift, smh_feat::kLayoutTimeMajor, d_fv, d_patches, d_maxkeys, stream);
}

// (the error texts of the shared checks keep the names of the entries they came with)
extern "C" int smh_plain_features_layout_f32(const smh_ctx *ctx, const float *d_S, int B, int T, int W, int shift, int patch_layout,
                                             float *d_fv, float *d_patches, int32_t *d_maxkeys, void *stream) {
    SMH_REQUIRE(layout_ok(patch_layout), "smh_plain_features_layout_f32: patch_layout must be 0 (image) or 1 (time-major), got %d",
                patch_layout);
    SMH_REQUIRE(ctx && d_S && d_fv && d_maxkeys, "smh_plain_features_f32: null argument");
    SMH_REQUIRE(B >= 0 && B <= 65535 && T >= 1, "smh_plain_features_f32: bad shape B=%d T=%d", B, T);
    int rc = check_context(ctx, "smh_plain_features_f32");
    if (rc) return rc;
    PatchOut po;
    rc = smh_feat::patch_out("smh_plain_features_f32", d_patches, false, T, W, shift, patch_layout, po);
    if (rc) return rc;
    if (B == 0) return po.nP;
    const int ntiles = (T + kTile - 1) / kTile;
    SMH_REQUIRE((long long)B * ntiles < (1ll << 31) - 8, "smh_plain_features_f32: B=%d clips of T=%d frames exceed one grid", B, T);
    hipStream_t st = (hipStream_t)stream;
    if (ctx->cfg.log_db) SMH_CHECK_HIP(hipMemsetAsync(d_maxkeys, 0, (size_t)B * sizeof(int32_t), st));
    Geo g;
    g.clips = nullptr, g.items = nullptr, g.n_items = B * ntiles;
    g.T = T, g.Ttiled = smh_tiled_frames(T, po.W), g.nP = po.nP, g.ntiles = ntiles;
    rc = launch_pair(ctx, d_S, d_fv, po, (int *)d_maxkeys, g, B, st);
    if (rc) return rc;
    return po.nP;
}

extern "C" size_t smh_plain_frontend_workspace_bytes(const smh_ctx *ctx, int B, int n_samples) {
    if (!ctx || B < 0) return 0;
    const int T = smh_num_frames(n_samples, ctx->cfg.n_fft, ctx->cfg.hop);
    if (T < 1) return 0;
    return align_up((size_t)B * ctx->K * T * sizeof(float), 256) + align_up((size_t)B * sizeof(int), 256);
}

extern "C" int smh_plain_frontend_f32(const smh_ctx *ctx, const float *d_audio, int B, int n_samples, int W, int shift, float *d_fv,
                                      float *d_patches, void *d_work, size_t work_bytes, float *d_S, void *stream) {
    return smh_plain_frontend_layout_f32(ctx, d_audio, B, n_samples, W, shift, smh_feat::kLayoutTimeMajor, d_fv, d_patches, d_work,
                                         work_bytes, d_S, stream);
}

extern "C" int smh_plain_frontend_layout_f32(const smh_ctx *ctx, const float *d_audio, int B, int n_samples, int W, int shift,
                                             int patch_layout, float *d_fv, float *d_patches, void *d_work, size_t work_bytes,
                                             float *d_S, void *stream) {
    SMH_REQUIRE(layout_ok(patch_layout), "smh_plain_frontend_layout_f32: patch_layout must be 0 (image) or 1 (time-major), got %d",
                patch_layout);
    SMH_REQUIRE(ctx && d_audio && d_fv && d_work, "smh_plain_frontend_f32: null argument");
    SMH_REQUIRE(B >= 0 && B <= 65535, "smh_plain_frontend_f32: B=%d out of range", B);
    const int T = smh_num_frames(n_samples, ctx->cfg.n_fft, ctx->cfg.hop);
    SMH_REQUIRE(T >= 1, "smh_plain_frontend_f32: clip of %d samples is shorter than n_fft=%d", n_samples, ctx->cfg.n_fft);
    SMH_REQUIRE(!d_patches || (W >= 1 && shift >= 1), "smh_plain_frontend_f32: bad patch geometry W=%d shift=%d", W, shift);
    int rc = check_context(ctx, "smh_plain_frontend_f32");
    if (rc) return rc;
    const size_t need = smh_plain_frontend_workspace_bytes(ctx, B, n_samples);
    if (work_bytes < need)
        return smh::set_error(SMH_E_WORKSPACE, "smh_plain_frontend_f32: workspace %zu < required %zu", work_bytes, need);
    const size_t spec = align_up((size_t)B * ctx->K * T * sizeof(float), 256);
    char *w = (char *)d_work;
    float *S = d_S ? d_S : (float *)w;
    int32_t *keys = (int32_t *)(w + spec);
    if (B == 0) return d_patches ? smh_num_patches(smh_tiled_frames(T, W), W, shift) : 0;
    rc = smh_stft_mag_f32(ctx, d_audio, B, n_samples, S, stream);
    if (rc) return rc;
    return smh_plain_features_layout_f32(ctx, S, B, T, W, shift, patch_layout, d_fv, d_patches, keys, stream);
}

// ---- ragged batches: the contract of smh_frontend_ragged_sizes / smh_frontend_ragged_f32, on the planner of smh_rag.h ----------------
namespace {

// device bytes one clip adds to a sub-batch: its descriptor, its max key, its (clip, tile) items of both stages (the STFT's counted
// at 16 frames, a lower bound of its tile) and its S
size_t plain_clip_bytes(const smh_ctx *ctx, int T) {
    const size_t items = (size_t)(T + 15) / 16 + (size_t)(T + kTile - 1) / kTile;
    return align_up((size_t)ctx->K * T, 4) * sizeof(float) + items * sizeof(Item) + sizeof(Clip) + sizeof(int);
}
constexpr size_t kPlainFixedBytes = 6 * 256;  // alignment slack between the regions of a sub-batch

int plain_sub_batch(const smh_ctx *ctx, const smh_stft::StftSwitches &sw, const float *d_audio, const HostClip *hc, int n, const PatchOut &po,
                    float *d_fv, char *d_work, size_t work_bytes, hipStream_t st) {
    std::vector<Clip> clips;
    const size_t spec = smh_rag::fill_clips(hc, n, ctx->K, po.patches != nullptr, clips);
    // the tables: [clips][stft items][projection items][max keys = 0]
    smh_rag::Tables t;
    Geo g;
    int n_stft;
    const size_t o_clips = t.add(clips.data(), clips.size() * sizeof(Clip));
    const size_t o_stft = t.add_items(hc, n, smh_stft::rag_frames(smh_stft::geom_of(ctx), sw, true), -1, &n_stft);
    const size_t o_proj = t.add_items(hc, n, kTile, -1, &g.n_items);
    const size_t o_keys = t.add(nullptr, (size_t)n * sizeof(int));
    int rc = t.upload(ctx, "smh_plain_frontend_ragged_f32", d_work, work_bytes, spec * sizeof(float), st);
    if (rc) return rc;
    float *d_S = reinterpret_cast<float *>(t.behind());
    g.clips = t.at<const Clip>(o_clips), g.items = t.at<const Item>(o_proj);
    rc = smh_stft::launch_rag(ctx, sw, d_audio, d_S, g.clips, t.at<const Item>(o_stft), n_stft, true, st);
    if (rc) return rc;
    g.T = g.Ttiled = g.nP = g.ntiles = 0;
    return launch_pair(ctx, d_S, d_fv, po, t.at<int>(o_keys), g, n, st);
}

}  // namespace

extern "C" int smh_plain_frontend_ragged_sizes(const smh_ctx *ctx, const long long *h_offsets, const int *h_lengths, int B, int W,
                                               int shift, long long *h_fv_off, long long *h_patch_off, int *h_T, int *h_nP,
                                               size_t *work_bytes) {
    SMH_REQUIRE(ctx && (B == 0 || (h_offsets && h_lengths)) && B >= 0, "smh_plain_frontend_ragged_sizes: bad argument");
    SMH_REQUIRE(W <= 0 || shift >= 1, "smh_plain_frontend_ragged_sizes: bad patch geometry W=%d shift=%d", W, shift);
    Layout p;
    int rc = smh_rag::plan_layout(ctx, "plain ragged", h_offsets, h_lengths, B, W, shift, W > 0, ctx->feat_rows, p);
    if (rc) return rc;
    smh_rag::export_layout(p, B, h_fv_off, h_patch_off, h_T, h_nP);
    if (work_bytes) {
        size_t total = kPlainFixedBytes, single = 0;
        for (int b = 0; b < B; ++b) {
            const size_t cb = plain_clip_bytes(ctx, p.T[b]);
            total += cb;
            single = std::max(single, std::max(cb + kPlainFixedBytes, smh_plain_frontend_workspace_bytes(ctx, 1, h_lengths[b])));
        }
        *work_bytes = smh_rag::work_size(B, single, total);
    }
    return SMH_OK;
}

extern "C" int smh_plain_frontend_ragged_f32(const smh_ctx *ctx, const float *d_audio, const long long *h_offsets,
                                             const int *h_lengths, int B, int W, int shift, float *d_fv, float *d_patches,
                                             void *d_work, size_t work_bytes, void *stream) {
    return smh_plain_frontend_ragged_layout_f32(ctx, d_audio, h_offsets, h_lengths, B, W, shift, smh_feat::kLayoutTimeMajor, d_fv,
                                                d_patches, d_work, work_bytes, stream);
}

extern "C" int smh_plain_frontend_ragged_layout_f32(const smh_ctx *ctx, const float *d_audio, const long long *h_offsets,
                                                    const int *h_lengths, int B, int W, int shift, int patch_layout, float *d_fv,
                                                    float *d_patches, void *d_work, size_t work_bytes, void *stream) {
    SMH_REQUIRE(layout_ok(patch_layout),
                "smh_plain_frontend_ragged_layout_f32: patch_layout must be 0 (image) or 1 (time-major), got %d", patch_layout);
    SMH_REQUIRE(ctx && d_audio && d_fv && d_work && h_offsets && h_lengths && B >= 0, "smh_plain_frontend_ragged_f32: bad argument");
    const bool patches = d_patches != nullptr;
    PatchOut po;
    int rc = smh_feat::patch_out("smh_plain_frontend_ragged_f32", d_patches, false, 0, W, shift, patch_layout, po);
    if (rc) return rc;
    SMH_REQUIRE((reinterpret_cast<uintptr_t>(d_work) % 16) == 0, "smh_plain_frontend_ragged_f32: the workspace must start on a 16-byte boundary");
    rc = check_context(ctx, "smh_plain_frontend_ragged_f32");
    if (rc) return rc;
    Layout p;
    rc = smh_rag::plan_layout(ctx, "plain ragged", h_offsets, h_lengths, B, W, shift, patches, ctx->feat_rows, p);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    // the specialised n_fft = 400 STFT needs every frame on an 8-byte boundary: a clip that starts elsewhere takes the generic kernel when
    // it is processed alone, so it is processed alone here too
    const smh_stft::StftSwitches sw = smh_stft::read_stft_switches();  // once per call: routing, table sizes and the launch agree
    const bool need8 = smh_stft::rag_needs_aligned8(smh_stft::geom_of(ctx), sw);
    auto taken = [&](int b) { return !need8 || smh_stft::clip_aligned8(reinterpret_cast<uintptr_t>(d_audio) + (uintptr_t)h_offsets[b] * 4); };
    std::vector<HostClip> hc;
    hc.reserve(B);
    for (int b = 0; b < B; ++b)
        if (taken(b)) hc.push_back(smh_rag::host_clip(p, h_offsets, b, po.W, 0));
    rc = smh_rag::run_sub_batches(
        hc.size(), kPlainFixedBytes, work_bytes, st, [&](size_t b) { return plain_clip_bytes(ctx, hc[b].T); }, [&](size_t b0, size_t nb) {
            return plain_sub_batch(ctx, sw, d_audio, hc.data() + b0, (int)nb, po, d_fv, (char *)d_work, work_bytes, st);
        });
    if (rc) return rc;
    // the clips off an 8-byte boundary, through smh_plain_frontend_f32 (the workspace is free again in stream order)
    return smh_rag::run_alone(p, B, W, shift, ctx->feat_rows, d_fv, d_patches, taken, [&](int b, int w, int sh, float *fv, float *pt) {
        return smh_plain_frontend_layout_f32(ctx, d_audio + h_offsets[b], 1, h_lengths[b], w, sh, patch_layout, fv, pt, d_work, work_bytes,
                                             nullptr, stream);
    });
}
