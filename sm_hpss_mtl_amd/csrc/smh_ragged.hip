// Ragged batches: clips of DIFFERENT lengths in one call, one launch per stage.
//
// The reference's generators process whole files of any length one by one (Proposed_Work_Results.py:92-95, 131-134, 189-192,
// 465-474 -> get_featuregram, lib/preprocessing.py:355-457, and get_feature_patches, :137-292).  Round 3 ran such a batch as a
// chain of seven B = 1 launches per file; here the host decides, from the lengths alone, a descriptor table (smh_rag::Clip) and a
// flat (clip, tile) work list per stage, uploads both in one copy, and every stage is ONE launch over all files:
//
//   stft400_kernel / stft_mag_kernel      items (clip, 20- or 16-frame tile)          audio -> S            (workspace)
//   hpss_median_split_kernel              items (clip, 76-frame tile + halo)          S -> harm (16-frame blocked), perc
//   clips whose featuregram fits an LDS image (smh_feat::clip_image_bytes: T <= 165 for 240 rows; smh_features_blocked_ok):
//     features_half_kernel<RAG> (even T) / features_clip_kernel<RAG> (odd T): the equal-length path's kernels, shapes per clip
//   longer clips, three streaming kernels of this file:
//     rag_walk_kernel     items (clip, 128-frame chunk): soft masks + mel sums -> fv (magnitudes), per-array maximum (atomicMax)
//     rag_stats_kernel    one wave per featuregram row: StandardScaler statistics of the dB row
//     rag_final_kernel    items (clip, 64-frame chunk): dB + top-dB floor -> fv (final), standardised time-major patches
//
// Bits: medians are selections and an STFT frame does not depend on its tile, so those stages give every clip what the equal-length
// entry points give it; the LDS-image clips run the same kernel code as smh_frontend_f32; the streaming kernels ARE what
// smh_frontend_f32 runs for clips beyond the LDS image (it builds the same tables for its B equal clips).  Clips no ragged kernel
// covers (a handful of frames, misaligned starts, window pairs without a block-split kernel) go through smh_frontend_f32 one by one.
#include <algorithm>
#include <cfloat>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "smh_common.h"
#include "smh_feat.h"
#include "smh_rag.h"

namespace smh_rag {

struct Staging {
    static constexpr int kSlots = 4;
    struct Slot {
        void *host = nullptr;
        size_t cap = 0;
        void *dev = nullptr;  // device twin of the slot, for the entries without a workspace of their own (launch_with_table)
        size_t dev_cap = 0;
        hipEvent_t ev = nullptr;
        bool in_flight = false;
    } slot[kSlots];
    int next = 0;
};

void destroy_staging(Staging *s) {
    if (!s) return;
    for (auto &sl : s->slot) {
        if (sl.ev) (void)hipEventDestroy(sl.ev);
        if (sl.host) (void)hipHostFree(sl.host);
        if (sl.dev) (void)hipFree(sl.dev);
    }
    delete s;
}

}  // namespace smh_rag

namespace {

using smh_feat::FeatPlan;
using smh_feat::final_value;
using smh_feat::floor_of_max;
using smh_feat::PatchOut;
using smh::xcd_item;
using smh_rag::align_up;
using smh_rag::Clip;
using smh_rag::HostClip;
using smh_rag::Item;
using smh_rag::Layout;
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int kWalkFrames = 128;  // frames per walk item: 64 lanes x a pair of frames
constexpr int kFinalFrames = 64;  // frames per finalisation item

// The next slot of the context's staging ring (four; call with rag_mu held), ready to take `bytes`: its event exists, whatever used
// it last -- a copy, or the kernel that read its device twin -- has completed (in practice it long has), and its pinned buffer, and
// with `twin` its device buffer too, hold at least `bytes`.
int acquire_slot(const smh_ctx *ctx, size_t bytes, bool twin, smh_rag::Staging::Slot **out) {
    if (!ctx->rag_staging) ctx->rag_staging = new smh_rag::Staging();
    smh_rag::Staging &sg = *ctx->rag_staging;
    smh_rag::Staging::Slot &sl = sg.slot[sg.next];
    sg.next = (sg.next + 1) % smh_rag::Staging::kSlots;
    if (!sl.ev) SMH_CHECK_HIP(hipEventCreateWithFlags(&sl.ev, hipEventDisableTiming));
    if (sl.in_flight) {
        SMH_CHECK_HIP(hipEventSynchronize(sl.ev));
        sl.in_flight = false;
    }
    const size_t cap = align_up(std::max<size_t>(bytes, 64 * 1024), 64 * 1024);
    if (sl.cap < bytes) {
        if (sl.host) SMH_CHECK_HIP(hipHostFree(sl.host));
        sl.host = nullptr, sl.cap = 0;
        SMH_CHECK_HIP(hipHostMalloc(&sl.host, cap, hipHostMallocDefault));
        sl.cap = cap;
    }
    if (twin && sl.dev_cap < bytes) {
        if (sl.dev) SMH_CHECK_HIP(hipFree(sl.dev));
        sl.dev = nullptr, sl.dev_cap = 0;
        SMH_CHECK_HIP(hipMalloc(&sl.dev, cap));
        sl.dev_cap = cap;
    }
    *out = &sl;
    return SMH_OK;
}

// host -> device copy of a call's tables through a pinned slot of the context
int stage_upload(const smh_ctx *ctx, const void *src, size_t bytes, void *d_dst, hipStream_t st) {
    std::lock_guard<std::mutex> lock(ctx->rag_mu);
    smh_rag::Staging::Slot *sl = nullptr;
    if (int rc = acquire_slot(ctx, bytes, false, &sl)) return rc;
    memcpy(sl->host, src, bytes);
    SMH_CHECK_HIP(hipMemcpyAsync(d_dst, sl->host, bytes, hipMemcpyHostToDevice, st));
    SMH_CHECK_HIP(hipEventRecord(sl->ev, st));
    sl->in_flight = true;
    return SMH_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// rag_walk_kernel: the bin walk of features_half_kernel (smh_feat.hip) for clips beyond the LDS image.  One workgroup per
// (clip, 128-frame chunk, half): nseg waves = row segments, lane = PAIR of frames; a wave walks the bins of its segment once,
// evaluates this half's soft mask  S own^2 / (own^2 + other^2)  per bin (lib/preprocessing.py:418; librosa.util.softmask with
// power 2) and adds it into the pending mel filters (:419-422); a finished filter's SUM goes to the featuregram row (the dB
// conversion needs the array's maximum, which only exists after the launch) and into the running maximum of its (clip, half) array.
// Even T: 8-byte loads and stores; odd T: two 4-byte accesses per pair, the lone last frame paired with itself.
// ---------------------------------------------------------------------------------------------------------------------------
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// Addresses in the walk are a buffer descriptor of the clip's array (four SGPRs, built from wave-uniform values), a wave-uniform
// byte offset of the row (soffset) and a 32-bit lane offset in bytes (voffset): buffer_load_dwordx2 v, v_off, s[rsrc], s_row offen.
// Written as plain pointers hipcc keeps a 64-bit pointer per lane and array and adds every row offset to it with a
// v_lshl_add_u64 (140 of them in the first version of this kernel, 13 spilled registers at 80 VGPRs).
template <bool EVEN>
__device__ __forceinline__ f32x2 load_pair(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff, unsigned d1) {
    if constexpr (EVEN) {
        const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0);
        return f32x2{__uint_as_float(v.x), __uint_as_float(v.y)};
    } else {
        return f32x2{__uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0)),
                     __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, voff + 4u * d1, soff, 0))};
    }
}

template <int NP, bool EVEN>
__device__ __forceinline__ void walk_pairs(const FeatPlan &fp, int seg, int half, int lane, int chunk, const float *S,
                                           const float *harmc, const float *perc, int K, int T, int rows, float *fvc, float &mx) {
    const int t0 = chunk * kWalkFrames + 2 * lane;
    const bool active = t0 < T;
    const int tp = min(t0, EVEN ? T - 2 : T - 1);  // this lane's pair starts here (an even frame)
    const unsigned d1 = (EVEN || tp + 1 < T) ? 1u : 0u;   // the second frame of the pair, or the first again
    const int m1 = fp.m1[seg], kbeg = fp.kbeg[seg], kend = fp.kend[seg];
    int mcur = fp.m0[seg];
    const float *plan = fp.plan + fp.off[seg];
    f32x2 acc[NP];
#pragma unroll
    for (int e = 0; e < NP; ++e) acc[e] = f32x2{0.f, 0.f};
    const unsigned spec_bytes = 4u * (unsigned)K * (unsigned)T, harm_bytes = 64u * (unsigned)K * (unsigned)((T + 15) >> 4);
    const __amdgpu_buffer_rsrc_t rS = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(S), 0, spec_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rP = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(perc), 0, spec_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rH = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(harmc), 0, harm_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rF = __builtin_amdgcn_make_buffer_rsrc(fvc, 0, 8u * (unsigned)rows * (unsigned)T, 0x00020000);
    // lane offsets: lo = the pair in a (K, T) row, ho = in bin 0 of the blocked harm image (T / 16, K, 16)
    const unsigned lo = 4u * (unsigned)tp, ho = 4u * (unsigned)((tp >> 4) * K * 16 + (tp & 15));
    // "own" = the median this half's mask favours (harm for H, perc for P), chosen once: descriptor, bin stride and lane offset
    const __amdgpu_buffer_rsrc_t r_own = half ? rP : rH, r_oth = half ? rH : rP;
    const unsigned own_st = half ? 4u * (unsigned)T : 64u, oth_st = half ? 64u : 4u * (unsigned)T;
    const unsigned own_lo = half ? lo : ho, oth_lo = half ? ho : lo;
    const unsigned row_bytes = 4u * (unsigned)T, fv_half = (unsigned)half * (unsigned)rows * row_bytes;
    auto emit_first = [&]() {
        const f32x2 v = acc[0];
        mx = fmaxf(mx, fmaxf(v.x, v.y));
        if (active) {
            const unsigned soff = fv_half + (unsigned)mcur * row_bytes;  // wave-uniform row
            if constexpr (EVEN) {
                __builtin_amdgcn_raw_buffer_store_b64(u32x2{__float_as_uint(v.x), __float_as_uint(v.y)}, rF, lo, soff, 0);
            } else {
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v.x), rF, lo, soff, 0);
                if (d1) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v.y), rF, lo + 4u, soff, 0);
            }
        }
#pragma unroll
        for (int e = 0; e + 1 < NP; ++e) acc[e] = acc[e + 1];
        acc[NP - 1] = f32x2{0.f, 0.f};
        ++mcur;
    };
    constexpr int kBatch = 8;  // bins of loads in flight per lane
    for (int k0 = kbeg; k0 < kend; k0 += kBatch) {
        f32x2 sv[kBatch], ov[kBatch], tv[kBatch];
        float4 wq[kBatch];
        int ne[kBatch];
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            const unsigned kk = (unsigned)min(k0 + u, K - 1);
            sv[u] = load_pair<EVEN>(rS, lo, kk * row_bytes, d1);
            ov[u] = load_pair<EVEN>(r_own, own_lo, kk * own_st, d1);
            tv[u] = load_pair<EVEN>(r_oth, oth_lo, kk * oth_st, d1);
            const int pi = min(k0 + u, kend - 1) - kbeg;  // wave-uniform: scalar loads
            wq[u] = *reinterpret_cast<const float4 *>(plan + (size_t)pi * 8);
            ne[u] = __float_as_int(plan[(size_t)pi * 8 + 4]);
        }
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            if (k0 + u >= kend) break;
            for (int i = 0; i < ne[u]; ++i) emit_first();
            const f32x2 own = ov[u], oth = tv[u];
            const f32x2 o2 = own * own;
            const f32x2 den = o2 + oth * oth;
            f32x2 X;
            constexpr float kDenMin = 7.8886091e-31f;  // 2^-100: below it (digital silence) the normalised form with its split_zeros rule
            if (__builtin_expect(__any(den.x < kDenMin || den.y < kDenMin), 0)) {
                auto one = [&](float s, float h, float p) {  // smh_softmask.h's softmask_pair_fast, this half's side only (called as that, the
                                                             // whole walk compiles to other code, not this branch alone)
                    float Z = fmaxf(h, p);
                    const bool bad = Z < FLT_MIN;
                    Z = bad ? 1.0f : Z;
                    const float iz = __builtin_amdgcn_rcpf(Z);
                    const float a = h * iz, b = p * iz;
                    const float m = a * a, r = b * b;
                    const float id = __builtin_amdgcn_rcpf(m + r);
                    const float mo = bad ? 0.5f : (half ? r : m) * id;
                    return s * mo;
                };
                X = f32x2{one(sv[u].x, half ? oth.x : own.x, half ? own.x : oth.x), one(sv[u].y, half ? oth.y : own.y, half ? own.y : oth.y)};
            } else {
                X = o2 * (sv[u] * f32x2{__builtin_amdgcn_rcpf(den.x), __builtin_amdgcn_rcpf(den.y)});
            }
            acc[0] += wq[u].x * X;
            acc[1] += wq[u].y * X;
            if constexpr (NP > 2) {
                acc[2] += wq[u].z * X;
                acc[3] += wq[u].w * X;
            }
        }
    }
    while (mcur < m1) emit_first();
}

// (80 VGPRs: three 8-wave workgroups per CU, like features_half_kernel -- the walk lives on loads in flight)
template <int NP>
__global__ void __launch_bounds__(512, 6)
rag_walk_kernel(FeatPlan fp, const float *__restrict__ S, const float *__restrict__ harmb, const float *__restrict__ perc, int K, int rows,
                float *__restrict__ fv, int *__restrict__ maxkeys, const Clip *__restrict__ clips, const Item *__restrict__ items,
                int n_items) {
    // item list entry n / 2, half n & 1: the two halves of a chunk read the same S / harm / perc and sit next to each other in
    // their XCD's dispatch order (the second one's loads come from that L2)
    unsigned n;
    if (!xcd_item(2 * n_items, n)) return;
    const Item item = items[n >> 1];
    const int half = n & 1;
    const Clip &c = clips[item.clip];
    const int T = c.T;
    const int seg = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    float mx = 0.f;  // sums of non-negative terms
    if (T & 1)
        walk_pairs<NP, false>(fp, seg, half, lane, item.tile, S + c.spec_off, harmb + c.harm_off, perc + c.spec_off, K, T, rows,
                              fv + c.fv_off, mx);
    else
        walk_pairs<NP, true>(fp, seg, half, lane, item.tile, S + c.spec_off, harmb + c.harm_off, perc + c.spec_off, K, T, rows,
                             fv + c.fv_off, mx);
    int key = __float_as_int(mx);  // non-negative floats order like their bit patterns
    for (int off = 32; off > 0; off >>= 1) key = max(key, __shfl_xor(key, off));
    if (lane == 0) atomicMax(&maxkeys[2 * item.clip + half], key);
}

// ---------------------------------------------------------------------------------------------------------------------------
// rag_stats_kernel: StandardScaler statistics of one featuregram row per wave (lib/preprocessing.py:211-214, 221-224: per row over
// the frames, population variance, constant rows left unscaled -- sklearn's _is_constant_feature / _handle_zeros_in_scale), in
// float64, on the final dB values, which are formed on the fly from the walk's sums.  Rows of all long clips of the call are numbered consecutively: clip list[i] owns rows i * R2 .. (i + 1) * R2 - 1.
// ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
rag_stats_kernel(const float *__restrict__ fv, const int *__restrict__ maxkeys, int log_db, int rows, const Clip *__restrict__ clips,
                 const int *__restrict__ list, int n_rows, float4 *__restrict__ stats) {
    const int lane = threadIdx.x & 63;
    const int rg = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (rg >= n_rows) return;
    const int R2 = 2 * rows;
    const int i = rg / R2, r = rg - i * R2;
    const int b = list[i];
    const Clip &c = clips[b];
    const int T = c.T;
    const float *x = fv + c.fv_off + (size_t)r * T;
    const float lim = floor_of_max(maxkeys[2 * b + (r >= rows ? 1 : 0)]);
    // one pass: sums of d = value - (the row's first value) and of d^2 in float64 (|d| <= 80 dB over at most 2^31 frames: the
    // shifted second moment loses nothing that a float32 patch could show)
    const double x0 = (double)final_value(x[0], lim, log_db);
    double s = 0.0, q = 0.0;
    for (int t = lane; t < T; t += 64) {
        const double d = (double)final_value(x[t], lim, log_db) - x0;
        s += d;
        q += d * d;
    }
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off), q += __shfl_xor(q, off);
    double mean, inv_scale;
    smh_feat::scaler_of_sums(x0, s, q, T, T, mean, inv_scale);  // (the constant-row rule counts the clip's own T frames here)
    // the f64 mean as hi + lo floats, 1 / scale as a float: what the LDS-image kernels keep per row as well
    if (lane == 0) stats[rg] = make_float4((float)mean, (float)(mean - (double)(float)mean), (float)inv_scale, 0.f);
}

// ---------------------------------------------------------------------------------------------------------------------------
// rag_final_kernel: one workgroup per (clip, 64-frame chunk).  Phase 1, a wave per row, lanes = frames: the walk's sum -> dB with the
// array's top-dB floor (librosa.power_to_db(x**2), lib/preprocessing.py:420,422) -> written back: the FINAL featuregram; with patches
// asked for, the standardised value goes to an LDS tile [row][frame] (odd stride).  Phase 2, a wave per frame, lanes = rows: the
// frame's column leaves the tile as one contiguous (2*rows)-float row of every patch that holds the frame -- tools.extract_patches'
// grid (lib/cython_impl/tools.pyx:21-38: patch p = frames p*shift .. p*shift + W - 1 of the tiled featuregram, frame index modulo T
// for clips shorter than a patch, lib/preprocessing.py:139-142), transposed to time-major (Proposed_Work_Results.py:235-236).
// IMAGE: the Conv2D models' layout (nP, 2*rows, W) instead (what extract_patches returns, lib/preprocessing.py:201-206).  Phase 2 then
// keeps phase 1's shape, a wave per row, lanes = the chunk's frames: lane tl holds frame v = t0 + tl, and for every patch p that holds
// v the wave stores tile[f][tl] at ((patch_off + p) * R2 + f) * W + (v - p * shift) -- consecutive lanes, consecutive floats of row f
// of the same patch (a patch boundary inside the chunk splits the run in two), read from consecutive words of one LDS row.  The
// patches a frame lies in are found once per lane, outside the loop over the rows.  Same tile, no LDS added; a separate
// instantiation, the time-major kernel keeps its registers.
// ---------------------------------------------------------------------------------------------------------------------------
template <bool IMAGE>
__global__ void __launch_bounds__(512)
rag_final_kernel(float *__restrict__ fv, const int *__restrict__ maxkeys, int log_db, int rows, int W, int shift,
                 float *__restrict__ patches, const float4 *__restrict__ stats, const Clip *__restrict__ clips,
                 const Item *__restrict__ items, int n_items) {
    extern __shared__ __attribute__((aligned(16))) float tile[];  // [R2][kFinalFrames + 1]
    unsigned n;
    if (!xcd_item(n_items, n)) return;
    const Item item = items[n];
    const Clip &c = clips[item.clip];
    const int T = c.T, R2 = 2 * rows;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    const int t0 = item.tile * kFinalFrames;
    const int nt = min(kFinalFrames, T - t0);
    constexpr int ld = kFinalFrames + 1;
    const bool want = patches != nullptr && c.nP > 0;
    const float limH = floor_of_max(maxkeys[2 * item.clip]), limP = floor_of_max(maxkeys[2 * item.clip + 1]);
    float *g = fv + c.fv_off + t0;
    constexpr int kB = 6;  // rows of loads in flight per wave
    for (int r0 = wave; r0 < R2; r0 += nw * kB) {
        float v[kB];
#pragma unroll
        for (int q = 0; q < kB; ++q) v[q] = g[(size_t)min(r0 + q * nw, R2 - 1) * T + min(lane, nt - 1)];
#pragma unroll
        for (int q = 0; q < kB; ++q) {
            const int r = r0 + q * nw;
            if (r < R2) {
                const float d = final_value(v[q], r < rows ? limH : limP, log_db);
                if (lane < nt) g[(size_t)r * T + lane] = d;
                if (want) {
                    const float4 st = stats[c.row0 + r];  // wave-uniform
                    // (x - mean) rounded to f32 as sklearn does (mean carried as hi + lo), then * 1/scale: std_patch_kernel's arithmetic
                    const float cv = (float)((double)d - ((double)st.x + (double)st.y));
                    tile[r * ld + lane] = cv * st.z;
                }
            }
        }
    }
    if (!want) return;
    __syncthreads();
    const int nP = c.nP, Tt = c.Ttiled;
    if constexpr (IMAGE) {
        if (lane >= nt) return;
        const size_t psz = (size_t)R2 * W;
        for (int v = t0 + lane; v < Tt; v += T) {  // the frame's positions in the tiled featuregram (one unless T < W)
            int p_lo, p_hi;
            smh_feat::patch_range(v, W, shift, nP, p_lo, p_hi);
            for (int p = p_lo; p <= p_hi; ++p) {
                float *o = patches + ((size_t)c.patch_off + p) * psz + (v - p * shift);
                for (int f = wave; f < R2; f += nw) o[(size_t)f * W] = tile[f * ld + lane];
            }
        }
        return;
    }
    for (int tl = wave; tl < nt; tl += nw) {
        for (int v = t0 + tl; v < Tt; v += T) {  // the frame's positions in the tiled featuregram (one unless T < W)
            int p_lo, p_hi;
            smh_feat::patch_range(v, W, shift, nP, p_lo, p_hi);
            for (int p = p_lo; p <= p_hi; ++p) {
                const int j = v - p * shift;
                float *o = patches + (((size_t)c.patch_off + p) * W + j) * R2;
                for (int f = lane; f < R2; f += 64) o[f] = tile[f * ld + tl];
            }
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------
// this file's rows of the kernel table (smh_feat.hip has the LDS-image kernels'): the instantiations the library holds
decltype(&rag_walk_kernel<2>) pick_walk_kernel(int pend) { return pend <= 2 ? rag_walk_kernel<2> : rag_walk_kernel<4>; }
decltype(&rag_final_kernel<false>) pick_final_kernel(bool image) { return image ? rag_final_kernel<true> : rag_final_kernel<false>; }

// (HostClip::cls here: 0: LDS image, even T; 1: LDS image, odd T; 2: streaming kernels)
struct RagGeom {
    int K, rows, stft_frames, med_frames;
    smh_stft::StftSwitches stft_sw;      // read once per call: the table sizes (stft_frames, med_frames) and the launches agree
    smh_median::MedianSwitches med_sw;
};

// device bytes one clip adds to a sub-batch (tables, statistics, S, perc, harm)
size_t clip_bytes(const RagGeom &g, const HostClip &c) {
    const size_t spec = align_up((size_t)g.K * c.T, 4) * sizeof(float);
    const size_t harm = (size_t)((c.T + 15) / 16) * 16 * g.K * sizeof(float);
    size_t items = (size_t)(c.T + g.stft_frames - 1) / g.stft_frames + (size_t)(c.T + g.med_frames - 1) / g.med_frames;
    size_t extra = sizeof(Clip) + 2 * sizeof(int) /* max keys */ + sizeof(int) /* list entry */;
    if (c.cls == 2) {
        items += (size_t)(c.T + kWalkFrames - 1) / kWalkFrames + (size_t)(c.T + kFinalFrames - 1) / kFinalFrames;
        extra += (size_t)2 * g.rows * sizeof(float4);
    }
    return 2 * spec + harm + items * sizeof(Item) + extra;
}
size_t final_tile_bytes(int rows) { return sizeof(float) * (size_t)2 * rows * (kFinalFrames + 1); }  // rag_final_kernel's [R2][65] tile
constexpr size_t kFixedBytes = 8 * 256;  // alignment slack between the regions of a sub-batch

bool rag_context_ok(const smh_ctx *ctx, const smh_median::MedianSwitches &msw) {
    if (!ctx->feat_walk_ok || smh::lab_env("SMH_FEAT_TAPS") || getenv("SMH_FEAT_TWO_KERNELS")) return false;
    if (ctx->feat_nseg[1] < 1 || ctx->feat_nseg[1] > 8) return false;
    if (final_tile_bytes(ctx->feat_rows) > 150 * 1024) return false;  // (this tile's own limit, not one of smh_feat.h's image budgets)
    return smh_rag::medians_ok(ctx, msw);
}
bool rag_clip_ok(const smh_ctx *ctx, int T) { return smh_rag::clip_ok(ctx, T); }

// one sub-batch: tables -> one upload -> one launch per stage
int run_sub_batch(const smh_ctx *ctx, const RagGeom &g, const float *d_audio, const HostClip *hc, int n, const PatchOut &po, float *d_fv,
                  char *d_work, size_t work_bytes, bool stft_aligned8, hipStream_t st) {
    float *const d_patches = po.patches;  // (po.nP is not used here: every kernel below reads a clip's nP from its Clip)
    std::vector<Clip> clips;
    const size_t spec = smh_rag::fill_clips(hc, n, g.K, d_patches != nullptr, clips);
    std::vector<int> list[3];
    size_t harm = 0;
    int max_T[2] = {0, 0};
    for (int b = 0; b < n; ++b) {
        const HostClip &h = hc[b];
        clips[b].harm_off = (long long)harm;
        clips[b].row0 = h.cls == 2 ? (int)list[2].size() * 2 * g.rows : 0;
        harm += (size_t)((h.T + 15) / 16) * 16 * g.K;
        if (h.cls != 2) max_T[h.cls] = std::max(max_T[h.cls], h.T);
        list[h.cls].push_back(b);
    }
    // the tables: [clips][stft items][median items][walk items][final items][lists 0, 1, 2][max keys = 0]
    smh_rag::Tables t;
    int n_stft, n_med, n_walk, n_final;
    const size_t o_clips = t.add(clips.data(), clips.size() * sizeof(Clip));
    const size_t o_stft = t.add_items(hc, n, g.stft_frames, -1, &n_stft), o_med = t.add_items(hc, n, g.med_frames, -1, &n_med);
    const size_t o_walk = t.add_items(hc, n, kWalkFrames, 2, &n_walk), o_final = t.add_items(hc, n, kFinalFrames, 2, &n_final);
    size_t o_list[3];
    for (int k = 0; k < 3; ++k) o_list[k] = t.add(list[k].data(), list[k].size() * sizeof(int));
    const size_t o_keys = t.add(nullptr, (size_t)2 * n * sizeof(int));
    // device regions behind the tables, each on a 256-byte boundary: stats, S, perc, harm
    const size_t stats_bytes = list[2].size() * (size_t)2 * g.rows * sizeof(float4);
    const size_t behind = align_up(stats_bytes, 256) + 2 * align_up(spec * sizeof(float), 256) + harm * sizeof(float);
    int rc = t.upload(ctx, "ragged front end", d_work, work_bytes, behind, st);
    if (rc) return rc;
    char *w = t.behind();
    auto region = [&](size_t bytes) {
        char *r = w;
        w += align_up(bytes, 256);
        return r;
    };
    float4 *d_stats = reinterpret_cast<float4 *>(region(stats_bytes));
    float *d_S = reinterpret_cast<float *>(region(spec * sizeof(float)));
    float *d_perc = reinterpret_cast<float *>(region(spec * sizeof(float)));
    float *d_harm = reinterpret_cast<float *>(w);
    const Clip *d_clips = t.at<const Clip>(o_clips);
    int *d_keys = t.at<int>(o_keys);
    rc = smh_stft::launch_rag(ctx, g.stft_sw, d_audio, d_S, d_clips, t.at<const Item>(o_stft), n_stft, stft_aligned8, st);
    if (rc) return rc;
    rc = smh_median::launch_rag(g.med_sw, d_S, d_harm, d_perc, g.K, ctx->cfg.l_harm, ctx->cfg.l_perc, d_clips, t.at<const Item>(o_med), n_med, st);
    if (rc) return rc;
    // (The LDS-image clips' small grids were tried on a side stream beside the streaming kernels: the fork / join events cost the host
    // 0.4 ms per call and the call got slower, 0.74 -> 1.10 ms per 256 files; everything stays on the caller's stream.)
    for (int k = 0; k < 2; ++k) {  // list 0: even T, list 1: odd T
        rc = smh_feat::launch_features_image(ctx, d_S, d_harm, d_perc, {(int)list[k].size(), max_T[k], d_clips, t.at<const int>(o_list[k]), k == 0},
                                             po, d_fv, nullptr, nullptr, st);
        if (rc < 0) return rc;
    }
    if (!list[2].empty()) {
        const FeatPlan fp = smh_feat::feat_plan(ctx, 1);
        const unsigned gw = smh::xcd_grid(2 * (long long)n_walk);
        hipLaunchKernelGGL(pick_walk_kernel(fp.pend), dim3(gw), dim3(64 * fp.nseg), 0, st, fp, d_S, d_harm, d_perc, g.K, g.rows, d_fv, d_keys,
                           d_clips, t.at<const Item>(o_walk), n_walk);
        rc = smh::launch_status("rag_walk_kernel");
        if (rc) return rc;
        if (d_patches) {
            const int n_rows = (int)list[2].size() * 2 * g.rows;
            hipLaunchKernelGGL(rag_stats_kernel, dim3((n_rows + 3) / 4), dim3(256), 0, st, (const float *)d_fv, (const int *)d_keys,
                               ctx->cfg.log_db, g.rows, d_clips, t.at<const int>(o_list[2]), n_rows, d_stats);
            rc = smh::launch_status("rag_stats_kernel");
            if (rc) return rc;
        }
        const size_t lds = final_tile_bytes(g.rows);
        const unsigned gf = smh::xcd_grid(n_final);
        rc = smh::launch_lds(pick_final_kernel(po.layout == smh_feat::kLayoutImage && d_patches), "rag_final_kernel", dim3(gf), dim3(512), lds,
                             lds, st, d_fv, (const int *)d_keys, ctx->cfg.log_db, g.rows, po.W, po.shift, d_patches, (const float4 *)d_stats,
                             d_clips, t.at<const Item>(o_final), n_final);
        if (rc) return rc;
    }
    return SMH_OK;
}

// all clips of `hc` through the ragged kernels, in as few sub-batches as the workspace allows
int run_rag(const smh_ctx *ctx, const float *d_audio, const std::vector<HostClip> &hc, const PatchOut &po, float *d_fv, void *d_work,
            size_t work_bytes, const smh_stft::StftSwitches &sw, const smh_median::MedianSwitches &msw, bool stft_aligned8, hipStream_t st) {
    if (hc.empty()) return SMH_OK;
    RagGeom g;
    g.K = ctx->K, g.rows = ctx->feat_rows, g.stft_sw = sw, g.med_sw = msw;
    g.stft_frames = smh_stft::rag_frames(smh_stft::geom_of(ctx), g.stft_sw, stft_aligned8);
    g.med_frames = smh_median::rag_tile_frames(ctx->K, ctx->cfg.l_harm, ctx->cfg.l_perc, g.med_sw);
    SMH_REQUIRE(g.med_frames > 0, "ragged front end: no median kernel for this context");
    return smh_rag::run_sub_batches(
        hc.size(), kFixedBytes, work_bytes, st, [&](size_t b) { return clip_bytes(g, hc[b]); }, [&](size_t b0, size_t nb) {
            return run_sub_batch(ctx, g, d_audio, hc.data() + b0, (int)nb, po, d_fv, (char *)d_work, work_bytes, stft_aligned8, st);
        });
}

}  // namespace

namespace smh_rag {

// ---- which clips the ragged STFT and median launches take (smh_rag.h) -------------------------------------------------------------
bool medians_ok(const smh_ctx *ctx, const smh_median::MedianSwitches &msw) {
    return !getenv("SMH_RAGGED_PERFILE") && smh_median::rag_tile_frames(ctx->K, ctx->cfg.l_harm, ctx->cfg.l_perc, msw) > 0;
}
// the block-split walkers fold once per side (windows of one have no walker)
bool clip_ok(const smh_ctx *ctx, int T) {
    // (the streaming kernels address a clip's rows with 32-bit offsets: K * T and 2 * rows * T below 2^29 elements -- a day of audio)
    if ((long long)(ctx->K + 16) * T >= (1ll << 29) || (long long)2 * ctx->feat_rows * T >= (1ll << 29)) return false;
    return smh_median::fast_ok(T, ctx->cfg.l_harm) && smh_median::fast_ok(ctx->K, ctx->cfg.l_perc);
}
bool start_ok(const smh_ctx *ctx, const smh_stft::StftSwitches &sw, const float *d_audio, long long off) {
    return !smh_stft::rag_needs_aligned8(smh_stft::geom_of(ctx), sw) ||
           smh_stft::clip_aligned8(reinterpret_cast<uintptr_t>(d_audio) + (uintptr_t)off * 4);
}

// ---- the planner (smh_rag.h) ------------------------------------------------------------------------------------------------
int plan_layout(const smh_ctx *ctx, const char *who, const long long *off, const int *len, int B, int W, int shift, bool patches,
                int fv_rows, Layout &p) {
    p.T.assign(B, 0), p.nP.assign(B, 0), p.fv_off.assign(B + 1, 0), p.patch_off.assign(B + 1, 0);
    for (int b = 0; b < B; ++b) {
        SMH_REQUIRE(off[b] >= 0 && len[b] >= 0, "%s: clip %d has a negative offset or length", who, b);
        const int T = smh_num_frames(len[b], ctx->cfg.n_fft, ctx->cfg.hop);
        SMH_REQUIRE(T >= 1, "%s: clip %d of %d samples is shorter than n_fft=%d", who, b, len[b], ctx->cfg.n_fft);
        p.T[b] = T;
        p.nP[b] = patches ? smh_num_patches(smh_tiled_frames(T, W), W, shift) : 0;
        p.fv_off[b + 1] = p.fv_off[b] + (long long)fv_rows * T;
        p.patch_off[b + 1] = p.patch_off[b] + p.nP[b];
    }
    return SMH_OK;
}

void export_layout(const Layout &p, int B, long long *h_fv_off, long long *h_patch_off, int *h_T, int *h_nP) {
    for (int b = 0; b <= B; ++b) {
        if (h_fv_off) h_fv_off[b] = p.fv_off[b];
        if (h_patch_off) h_patch_off[b] = p.patch_off[b];
    }
    for (int b = 0; b < B; ++b) {
        if (h_T) h_T[b] = p.T[b];
        if (h_nP) h_nP[b] = p.nP[b];
    }
}

size_t work_size(int B, size_t single, size_t total) {
    constexpr size_t kWorkCap = (size_t)8 << 30;
    return B == 0 ? 0 : align_up(std::max(single, std::min(total, kWorkCap)), 256);
}

HostClip host_clip(const Layout &p, const long long *off, int b, int W, int cls) {
    return {off[b], p.fv_off[b], p.patch_off[b], p.T[b], smh_tiled_frames(p.T[b], W), p.nP[b], cls};
}

size_t fill_clips(const HostClip *hc, int n, int K, bool patches, std::vector<Clip> &clips) {
    clips.assign(n, Clip{});
    size_t spec = 0;
    for (int b = 0; b < n; ++b) {
        const HostClip &h = hc[b];
        Clip &c = clips[b];
        c.audio_off = h.audio_off, c.fv_off = h.fv_off, c.patch_off = h.patch_off, c.spec_off = (long long)spec;
        c.T = h.T, c.Ttiled = h.Ttiled, c.nP = patches ? h.nP : 0;
        spec += align_up((size_t)K * h.T, 4);
    }
    return spec;
}

size_t Tables::add(const void *src, size_t bytes) {
    const size_t o = blob_.size();
    blob_.resize(align_up(o + bytes, 16), 0);
    if (src && bytes) memcpy(blob_.data() + o, src, bytes);
    return o;
}

size_t Tables::add_items(const HostClip *hc, int n, int frames, int cls, int *count) {
    size_t k = 0;
    for (int b = 0; b < n; ++b)
        if (cls < 0 || hc[b].cls == cls) k += (size_t)(hc[b].T + frames - 1) / frames;
    const size_t o = add(nullptr, k * sizeof(Item));
    Item *it = reinterpret_cast<Item *>(blob_.data() + o);
    for (int b = 0; b < n; ++b)
        if (cls < 0 || hc[b].cls == cls)
            for (int t = 0, i = 0; t < hc[b].T; t += frames, ++i) *it++ = {b, i};
    *count = (int)k;
    return o;
}

int Tables::upload(const smh_ctx *ctx, const char *who, char *d_work, size_t work_bytes, size_t behind, hipStream_t st) {
    d_ = d_work;
    const size_t need = align_up(blob_.size(), 256) + behind;
    if (need > work_bytes) return smh::set_error(SMH_E_WORKSPACE, "%s: workspace %zu < %zu needed by a single clip", who, work_bytes, need);
    return stage_upload(ctx, blob_.data(), blob_.size(), d_work, st);
}

int run_sub_batches(size_t n, size_t fixed, size_t work_bytes, hipStream_t st,
                    const std::function<size_t(size_t)> &bytes, const std::function<int(size_t, size_t)> &run) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone)
        return smh::set_error(SMH_E_INVALID, "the ragged front end uploads its tables from a staging buffer: it cannot be captured in a graph");
    size_t b0 = 0;
    while (b0 < n) {
        size_t need = fixed, b1 = b0;
        while (b1 < n) {
            const size_t cb = bytes(b1);
            if (b1 > b0 && need + cb > work_bytes) break;
            need += cb;
            ++b1;
        }
        int rc = run(b0, b1 - b0);
        if (rc) return rc;
        b0 = b1;
    }
    return SMH_OK;
}

int launch_with_table(const smh_ctx *ctx, const char *who, const void *src, size_t bytes, hipStream_t st,
                      const std::function<int(const void *)> &launch) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone)
        return smh::set_error(SMH_E_INVALID, "%s uploads its table from a staging buffer: it cannot be captured in a graph", who);
    std::lock_guard<std::mutex> lock(ctx->rag_mu);
    Staging::Slot *sl = nullptr;
    if (int rc = acquire_slot(ctx, bytes, true, &sl)) return rc;
    memcpy(sl->host, src, bytes);
    SMH_CHECK_HIP(hipMemcpyAsync(sl->dev, sl->host, bytes, hipMemcpyHostToDevice, st));
    const int rc = launch(sl->dev);
    SMH_CHECK_HIP(hipEventRecord(sl->ev, st));  // behind the kernel (also after a failed launch: the copy is enqueued)
    sl->in_flight = true;
    return rc;
}

int run_alone(const Layout &p, int B, int W, int shift, int fv_rows, float *d_fv, float *d_patches, const std::function<bool(int)> &taken,
              const std::function<int(int, int, int, float *, float *)> &alone) {
    const size_t prow = (size_t)(W > 0 ? W : 0) * fv_rows;
    for (int b = 0; b < B; ++b) {
        if (taken(b)) continue;
        float *pt = d_patches && p.nP[b] > 0 ? d_patches + (size_t)p.patch_off[b] * prow : nullptr;
        int rc = alone(b, pt ? W : 0, pt ? shift : 0, d_fv + p.fv_off[b], pt);
        if (rc < 0) return rc;
    }
    return SMH_OK;
}

// ---- smh_frontend_f32's route for B equal clips beyond the LDS image (smh_rag.h) -----------------------------------------------
size_t equal_overhead_bytes(const smh_ctx *ctx, int B, int T) {
    RagGeom g;
    g.K = ctx->K, g.rows = ctx->feat_rows, g.stft_frames = 16, g.med_frames = 16;  // (upper bounds of the item counts)
    HostClip h;
    h.T = T, h.cls = 2;
    const size_t spec = align_up((size_t)g.K * T, 4) * sizeof(float);
    const size_t harm = (size_t)((T + 15) / 16) * 16 * g.K * sizeof(float);
    return (size_t)B * (clip_bytes(g, h) - 2 * spec - harm) + kFixedBytes + 4 * 256 + (size_t)B * 16;
}

int run_equal(const smh_ctx *ctx, const float *d_audio, int B, int n_samples, int T, const PatchOut &po, float *d_fv, void *d_work,
              size_t work_bytes, const smh_median::MedianSwitches &msw, bool stft_aligned8, hipStream_t st) {
    if (!rag_context_ok(ctx, msw) || !rag_clip_ok(ctx, T) || (reinterpret_cast<uintptr_t>(d_work) % 16) != 0) return 0;
    const int rows2 = 2 * ctx->feat_rows;
    std::vector<HostClip> hc(B);
    for (int b = 0; b < B; ++b) {
        hc[b].audio_off = (long long)b * n_samples, hc[b].fv_off = (long long)b * rows2 * T, hc[b].patch_off = (long long)b * po.nP;
        hc[b].T = T, hc[b].Ttiled = smh_tiled_frames(T, po.W), hc[b].nP = po.nP, hc[b].cls = 2;
    }
    int rc = run_rag(ctx, d_audio, hc, po, d_fv, d_work, work_bytes, smh_stft::read_stft_switches(), msw, stft_aligned8, st);
    return rc ? rc : 1;
}

int feature_route(const smh_ctx *ctx, const smh_median::MedianSwitches &msw, int T) {
    if (smh_features_blocked_ok(ctx, T, 0)) {
        if (!smh_median::blocked_harm_ok(ctx->K, T, ctx->cfg.l_harm, ctx->cfg.l_perc, msw)) return 3;
        return ((T & 1) || getenv("SMH_FEAT_NOPAIR")) ? 1 : 0;
    }
    return rag_context_ok(ctx, msw) && rag_clip_ok(ctx, T) ? 2 : 3;
}

}  // namespace smh_rag

// tests: the feature route (smh_rag::feature_route) of a clip of T frames in this context; -1 for a bad argument
extern "C" int smh_internal_frontend_route(const smh_ctx *ctx, int T) {
    if (!ctx || T < 1) return -1;
    return smh_rag::feature_route(ctx, smh_median::read_median_switches(), T);
}

// ---- the C ABI -------------------------------------------------------------------------------------------------------------
namespace {
// which clips the ragged kernels take (cls 0 / 1 / 2) and which go through smh_frontend_f32 alone (-1)
void classify(const smh_ctx *ctx, const smh_stft::StftSwitches &sw, const smh_median::MedianSwitches &msw, const float *d_audio, const long long *off, const Layout &p, int B,
              std::vector<int> &cls) {
    cls.assign(B, -1);
    if (!rag_context_ok(ctx, msw)) return;
    // the specialised STFT needs every frame on an 8-byte boundary: a clip that starts elsewhere takes the generic kernel when it is
    // processed alone, so it is processed alone here too (same bits either way)
    for (int b = 0; b < B; ++b) {
        if (!rag_clip_ok(ctx, p.T[b])) continue;
        if (!smh_rag::start_ok(ctx, sw, d_audio, off[b])) continue;
        // (even T: one workgroup per clip half; odd T -- or SMH_FEAT_NOPAIR -- one per clip: the route smh_frontend_f32 takes)
        const int r = smh_rag::feature_route(ctx, msw, p.T[b]);
        if (r <= 2) cls[b] = r;
    }
}
}  // namespace

extern "C" int smh_frontend_ragged_sizes(const smh_ctx *ctx, const long long *h_offsets, const int *h_lengths, int B, int W,
                                         int shift, long long *h_fv_off, long long *h_patch_off, int *h_T, int *h_nP,
                                         size_t *work_bytes) {
    SMH_REQUIRE(ctx && (B == 0 || (h_offsets && h_lengths)) && B >= 0, "smh_frontend_ragged_sizes: bad argument");
    SMH_REQUIRE(W <= 0 || shift >= 1, "smh_frontend_ragged_sizes: bad patch geometry W=%d shift=%d", W, shift);
    Layout p;
    int rc = smh_rag::plan_layout(ctx, "ragged", h_offsets, h_lengths, B, W, shift, W > 0, 2 * ctx->feat_rows, p);
    if (rc) return rc;
    smh_rag::export_layout(p, B, h_fv_off, h_patch_off, h_T, h_nP);
    if (work_bytes) {
        // every clip the ragged kernels take at once, and never less than the largest single clip needs (alone in a sub-batch, or
        // through smh_frontend_f32): smh_rag::work_size
        std::vector<int> cls;
        const smh_median::MedianSwitches msw = smh_median::read_median_switches();
        classify(ctx, smh_stft::read_stft_switches(), msw, nullptr, h_offsets, p, B, cls);  // (alignment is the call's business: sized as if every clip qualified)
        RagGeom g;
        g.K = ctx->K, g.rows = ctx->feat_rows, g.stft_frames = 16;
        g.med_frames = std::max(16, smh_median::rag_tile_frames(ctx->K, ctx->cfg.l_harm, ctx->cfg.l_perc, msw));
        size_t total = kFixedBytes, single = 0;
        for (int b = 0; b < B; ++b) {
            single = std::max(single, smh_frontend_workspace_bytes(ctx, 1, h_lengths[b]));
            if (cls[b] < 0) continue;
            HostClip h;
            h.T = p.T[b], h.cls = cls[b];
            const size_t cb = clip_bytes(g, h);
            total += cb;
            single = std::max(single, cb + kFixedBytes);
        }
        *work_bytes = smh_rag::work_size(B, single, total);
    }
    return SMH_OK;
}

extern "C" int smh_frontend_ragged_layout_f32(const smh_ctx *ctx, const float *d_audio, const long long *h_offsets,
                                              const int *h_lengths, int B, int W, int shift, int patch_layout, float *d_fv,
                                              float *d_patches, void *d_work, size_t work_bytes, void *stream) {
    SMH_REQUIRE(ctx && d_audio && d_fv && d_work && h_offsets && h_lengths && B >= 0, "smh_frontend_ragged_f32: bad argument");
    SMH_REQUIRE(patch_layout == smh_feat::kLayoutImage || patch_layout == smh_feat::kLayoutTimeMajor,
                "smh_frontend_ragged_layout_f32: patch_layout must be 0 (image) or 1 (time-major), got %d", patch_layout);
    const bool patches = d_patches != nullptr;
    PatchOut po;
    int rc = smh_feat::patch_out("smh_frontend_ragged_f32", d_patches, false, 0, W, shift, patch_layout, po);
    if (rc) return rc;
    SMH_REQUIRE((reinterpret_cast<uintptr_t>(d_work) % 16) == 0, "smh_frontend_ragged_f32: the workspace must start on a 16-byte boundary");
    Layout p;
    rc = smh_rag::plan_layout(ctx, "ragged", h_offsets, h_lengths, B, W, shift, patches, 2 * ctx->feat_rows, p);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const smh_stft::StftSwitches sw = smh_stft::read_stft_switches();  // once per call: routing, table sizes and the launch agree
    const smh_median::MedianSwitches msw = smh_median::read_median_switches();
    std::vector<int> cls;
    classify(ctx, sw, msw, d_audio, h_offsets, p, B, cls);
    std::vector<HostClip> hc;
    hc.reserve(B);
    for (int b = 0; b < B; ++b)
        if (cls[b] >= 0) hc.push_back(smh_rag::host_clip(p, h_offsets, b, po.W, cls[b]));
    rc = run_rag(ctx, d_audio, hc, po, d_fv, d_work, work_bytes, sw, msw, true, st);
    if (rc) return rc;
    // the clips no ragged kernel covers, one by one on the same stream (the workspace is free again in stream order)
    return smh_rag::run_alone(p, B, W, shift, 2 * ctx->feat_rows, d_fv, d_patches, [&](int b) { return cls[b] >= 0; },
                              [&](int b, int w, int sh, float *fv, float *pt) {
                                  return smh_frontend_layout_f32(ctx, d_audio + h_offsets[b], 1, h_lengths[b], w, sh, patch_layout, fv, pt,
                                                                 d_work, work_bytes, nullptr, nullptr, nullptr, stream);
                              });
}

extern "C" int smh_frontend_ragged_f32(const smh_ctx *ctx, const float *d_audio, const long long *h_offsets,
                                       const int *h_lengths, int B, int W, int shift, float *d_fv, float *d_patches,
                                       void *d_work, size_t work_bytes, void *stream) {
    return smh_frontend_ragged_layout_f32(ctx, d_audio, h_offsets, h_lengths, B, W, shift, smh_feat::kLayoutTimeMajor, d_fv, d_patches,
                                          d_work, work_bytes, stream);
}
