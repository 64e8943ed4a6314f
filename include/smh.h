/* smh.h -- C ABI of libsmh.so: the MI355X (gfx950) implementation of the SM_HPSS_MTL hot path.
 *
 * The reference (mrinmoy-iitg/SM_HPSS_MTL) has NO C ABI of its own: its hot path is a Python call
 * surface over librosa / scipy / sklearn / a Cython module / Keras.  Each entry point below therefore
 * cites the reference Python call it replaces (paths under /root/reference).  INTEGRATION.md shows
 * the ctypes stub a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer named `d_*` is DEVICE memory owned by the caller (e.g. torch tensors); the
 *     library never allocates or frees caller buffers and keeps no global state besides the
 *     immutable tables owned by an explicit `smh_ctx` / `smh_model`;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); all work is stream-ordered,
 *     nothing synchronises, so every call is hipGraph-capturable;
 *   - spectrogram-like tensors are (B, rows, T) row-major float32 -- per clip exactly the (K, T)
 *     arrays librosa returns;
 *   - return value: 0 = ok, <0 = error (SMH_E_*); smh_last_error() gives a thread-local message.
 *   - no CPU fallback exists: without a HIP device every compute entry point fails with SMH_E_HIP.
 */
#ifndef SMH_H
#define SMH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMH_OK 0
#define SMH_E_INVALID (-1)   /* bad argument / unsupported size            */
#define SMH_E_HIP (-2)       /* HIP runtime error (launch, alloc, no GPU)  */
#define SMH_E_WORKSPACE (-3) /* caller workspace too small                 */
#define SMH_E_DEVICE (-4)    /* a kernel reported through the object's device error word that its outputs are not results */

#define SMH_MAX_MEDIAN 63 /* largest supported (odd) median window        */

typedef struct smh_ctx smh_ctx;     /* front-end constant tables (window, twiddles, mel CSR)   */
typedef struct smh_model smh_model; /* B3_MTL descriptor + packed device weights              */

/* PARAMS keys the front end reads (Proposed_Work_Results.py:726-728,758-773,800-801). */
typedef struct smh_frontend_cfg {
    int32_t n_fft;      /* PARAMS['n_fft'][Model]: 400 (Jang: 512)                          */
    int32_t win_length; /* int(Tw*fs/1000): 400                                             */
    int32_t hop;        /* int(Ts*fs/1000): 160                                             */
    int32_t n_mels;     /* PARAMS['n_mels'][Model]: 120; <=0 -> no mel projection (rows=K)  */
    int32_t l_harm;     /* PARAMS['l_harm'][Model]: 21 (median along frames)                */
    int32_t l_perc;     /* PARAMS['l_perc'][Model]: 11 (median along bins)                  */
    int32_t log_db;     /* 1 -> librosa.power_to_db(x**2) ('Log*' feature names)            */
    float mel_sr;       /* librosa default 22050 (the reference never passes sr)            */
} smh_frontend_cfg;

const char *smh_last_error(void);
int smh_version(void);
int smh_device_count(void); /* 0 when no HIP device is visible */

int smh_ctx_create(const smh_frontend_cfg *cfg, smh_ctx **out); /* = smh_ctx_create_ex(cfg, SMH_STFT_F32, out) */
/* STFT precision of a context.  Everything after the STFT (medians, masks, mel, dB, scaler, patches) reads the same f32 S in
 * both modes; only how |S| is computed differs.  smh_stft_mag_f32, smh_frontend_f32 (the streaming route included) and
 * smh_frontend_ragged_f32 dispatch on it.
 *   SMH_STFT_F32 (default): f32 FFT, |z| on the hardware square root.  |S| is within 1e-5 of max|S| of the reference's; the
 *                 last bits of small bins differ.  The faster mode.
 *   SMH_STFT_F64: x[n] = w64[n] * (double)y[t*hop + n] with the f64 periodic Hann window, an f64 FFT with f64 twiddles from
 *                 exactly reduced angles, Re and Im rounded once to f32 (nearest even), then numpy's complex64 magnitude
 *                 l = max(|re|, |im|), r = min(..) / l, |z| = l * sqrtf(fmaf(r, r, 1)) (0 when l = 0), in IEEE f32.
 *                 |S| equals np.abs(librosa.core.stft(y, n_fft, win_length, hop, center=False)) (float64 rfft -> complex64
 *                 -> np.abs) bit for bit on (practically) every bin: the f64 transform's summation order does not survive
 *                 the rounding to complex64.  The exception: bins more than ~100 dB below their frame's maximum (near-pure
 *                 tones).  There the f64 rounding noise of any order but pocketfft's reaches the f32 ulp; such bins are within
 *                 1e-11 of the frame's maximum.  The f64 window and twiddle tables exist only in such a context; an n_fft
 *                 whose f64 frame does not fit the kernel's LDS is rejected here (SMH_E_INVALID), never run in f32.
 * Any other stft_precision: SMH_E_INVALID. */
#define SMH_STFT_F32 0
#define SMH_STFT_F64 1
int smh_ctx_create_ex(const smh_frontend_cfg *cfg, int stft_precision, smh_ctx **out);
void smh_ctx_destroy(smh_ctx *ctx);
/* rows of one half (harmonic or percussive) of the featuregram: n_mels, or K = 1+n_fft/2 */
int smh_ctx_feat_rows(const smh_ctx *ctx);
/* copies the (n_mels, K) float32 mel basis to HOST memory (for inspection / tests) */
int smh_ctx_mel_basis(const smh_ctx *ctx, float *h_out);

/* ---- integer contracts (host, exact) ------------------------------------------------------- */
/* librosa util.frame, center=False: 1 + (N - n_fft)/hop, 0 if N < n_fft */
int smh_num_frames(int n_samples, int n_fft, int hop);
/* get_feature_patches tiling (lib/preprocessing.py:139-142): frames after `while T<=W: append` */
int smh_tiled_frames(int T, int W);
/* tools.extract_patches (lib/cython_impl/tools.pyx:24-29): len(range(W/2, T-W/2, shift)) */
int smh_num_patches(int T, int W, int shift);
/* start frame of patch p (tools.pyx:30-34) */
int smh_patch_start(int T, int W, int shift, int p);

/* ---- a1: np.abs(librosa.core.stft(y, n_fft, win_length, hop_length, center=False)) ----------
 * lib/preprocessing.py:407,417,429,439.  d_audio (B, n_samples) -> d_S (B, K, T).  In the context's STFT precision
 * (smh_ctx_create_ex): f32, or f64 with a bit-exact |S|.                                                                   */
int smh_stft_mag_f32(const smh_ctx *ctx, const float *d_audio, int B, int n_samples, float *d_S, void *stream);

/* ---- a2: the two median filters inside librosa.decompose.hpss (preprocessing.py:408,418,...) --
 * harm = median_filter(S, (1,l_harm), 'reflect');  perc = median_filter(S, (l_perc,1), 'reflect').
 * Bit-exact selection.  smh_hpss_median_f32 computes both in ONE launch ("the median kernel").   */
int smh_hpss_median_f32(const smh_ctx *ctx, const float *d_S, int B, int K, int T, int l_harm, int l_perc,
                        float *d_harm, float *d_perc, void *stream);
int smh_median_time_f32(const smh_ctx *ctx, const float *d_S, int B, int K, int T, int l_harm, float *d_harm,
                        void *stream);
int smh_median_freq_f32(const smh_ctx *ctx, const float *d_S, int B, int K, int T, int l_perc, float *d_perc,
                        void *stream);

/* Layout-aware variants used by the fused pipeline (no reference counterpart: the reference never
 * materialises harm on a device).  harm_layout 0 = (B,K,T) as above; 1 = (B,T,K) time-major, which lets
 * the harmonic lanes (one per bin) store coalesced -- about 30 us per 1024 clips faster on MI355X.
 * smh_hpss_median_ex_f32 returns the layout it actually wrote; pass that value on to smh_features_ex_f32.
 * It falls back to 0 for window pairs or tiny axes outside the fused kernel table, and it writes 1 for a
 * requested 2 wherever no block-split kernel runs: a window above 21 (pairs such as (31,31) or (11,51),
 * single windows from 23), or a spectrogram so tall (K of several hundred bins and more) that the bins
 * alone exceed the block-split kernel's waves.  B == 0 returns the requested layout.                  */
int smh_hpss_median_ex_f32(const smh_ctx *ctx, const float *d_S, int B, int K, int T, int l_harm, int l_perc,
                           float *d_harm, float *d_perc, int harm_layout, void *stream);
/* the harmonic median alone (= smh_median_time_f32) in any of those layouts; returns the layout written */
int smh_median_time_ex_f32(const smh_ctx *ctx, const float *d_S, int B, int K, int T, int l_harm, float *d_harm,
                           int harm_layout, void *stream);

/* ---- a3: H = S*softmask(harm,perc), P = S*softmask(perc,harm); power=2, split_zeros=True ---- */
int smh_softmask_f32(const smh_ctx *ctx, const float *d_S, const float *d_harm, const float *d_perc, size_t n,
                     float *d_H, float *d_P, void *stream);

/* ---- a3': HPSS audio separation -- librosa.effects.hpss with this library's framing; what makes the reference's hpss_audio/
 * listening demos (<name>, <name>_Harmonic, <name>_Percussive).  With w the context's window (periodic Hann of win_length,
 * zero-padded centrally to n_fft), center=False and T = smh_num_frames(n_samples, n_fft, hop):
 *   D[:, t] = rfft(w * y[t*hop : t*hop + n_fft]);   D_h = D * softmask(harm, perc),  D_p = D * softmask(perc, harm)
 *   (power 2, split_zeros, margin 1: |D_h|, |D_p| are smh_softmask_f32's H and P; the mixture's phase is kept);
 *   y_c = librosa.istft(D_c, center=False, length=n_samples):  num[n] = sum_t w[n - t*hop] * irfft(D_c[:, t])[n - t*hop],
 *   wss[n] = sum_t w^2[n - t*hop],  y_c[n] = num[n] / wss[n] where wss[n] > FLT_MIN, else num[n]; 0 from n_fft + hop*(T-1) on.
 * smh_hpss_resynth_f32: the one kernel, on caller-supplied medians.  d_audio (B, n_samples), d_harm, d_perc (B, K, T) ->
 *   d_y_harm, d_y_perc (B, n_samples).  The transforms are f32 in either STFT precision; the complex spectrogram stays on chip.
 *   No atomics: a sample is the sum of its frames in ascending order, so a clip's samples are bit for bit the same alone, at any
 *   place of any batch and in every run.
 * smh_hpss_audio_f32: smh_stft_mag_f32 -> smh_hpss_median_f32 (the context's l_harm, l_perc) -> smh_hpss_resynth_f32, with S,
 *   harm and perc in d_work (smh_hpss_audio_workspace_bytes, 16-byte aligned).  The context's STFT precision governs |S|, and with
 *   it the medians, only.  (The f32 STFT picks its kernel by the clips' alignment: in a batch of an ODD n_samples its |S| differs
 *   in the last bits from the same clip's alone, as smh_stft_mag_f32's does; even lengths and the f64 STFT are batch-independent.)
 * Refused with SMH_E_INVALID (text in smh_last_error) before any launch: null pointers; B < 0; B > 65535 (the grid limit);
 * n_samples < n_fft (no frame to invert); outputs that overlap an input, the workspace or each other; hop > n_fft; n_fft > 17 * hop
 * (more than 17 frames per sample); a tile that does not fit the kernel's LDS (150 KB: csrc/smh_resynth_plan.h; both of the
 * reference's configurations, (400, 400, 160) and (512, 400, 160), take 55 and 65 KB).  A workspace that is too small: SMH_E_WORKSPACE.  B == 0 returns SMH_OK and touches nothing.  Every offset is 64-bit. */
int smh_hpss_resynth_f32(const smh_ctx *ctx, const float *d_audio, int B, int n_samples, const float *d_harm, const float *d_perc,
                         float *d_y_harm, float *d_y_perc, void *stream);
size_t smh_hpss_audio_workspace_bytes(const smh_ctx *ctx, int B, int n_samples);
int smh_hpss_audio_f32(const smh_ctx *ctx, const float *d_audio, int B, int n_samples, float *d_y_harm, float *d_y_perc,
                       void *d_work, size_t work_bytes, void *stream);

/* ---- a3' for clips of DIFFERENT lengths in one call (the layout of the ragged front ends below: HOST arrays h_offsets, h_lengths).
 * Clip b is h_lengths[b] samples at float h_offsets[b] of d_audio; its two components go to the same offsets of d_y_harm and
 * d_y_perc, and the floats between clips are not written.  ONE LAUNCH PER STAGE for all clips: the STFT of every clip in the context's
 * precision, both medians, the resynthesis kernel in its ragged form, on a descriptor table and (clip, tile) work lists uploaded in
 * one copy from a pinned slot of the context.  The medians write harm in 16-frame blocks and the resynthesis reads it there.
 * CONTRACT: every clip's two components are bit for bit what smh_hpss_audio_f32 gives that clip alone (B = 1, at its address),
 * whatever else is in the call, whatever the sub-batching, in every run.  No atomics.
 * Clips the ragged kernels do not cover go through smh_hpss_audio_f32 one by one on the same stream, same result in the same place:
 * every clip of a context without a block-split median kernel (a window above 21) or under SMH_RAGGED_PERFILE; a clip with T <=
 * l_harm / 2 + 4 frames (or K <= l_perc / 2 + 4 bins); a clip that starts off an 8-byte boundary where the f32 STFT reads float2
 * (n_fft = 400, even hop: keep every offset a multiple of 4 samples); a clip beyond 32-bit row offsets (2^29 elements).
 * smh_hpss_audio_ragged_sizes: h_T (or NULL) gets every clip's frames, *work_bytes (or NULL) the workspace that takes every clip at
 *   once -- tables, then S, perc and blocked harm of every clip --, at most 8 GiB and never less than the largest single clip needs
 *   (smh_hpss_audio_workspace_bytes(ctx, 1, len) included).  A smaller workspace that still holds the largest single clip (what
 *   _sizes answers for that clip alone) runs the call in sub-batches, same bits; below that: SMH_E_WORKSPACE.
 * Refused with SMH_E_INVALID before anything is enqueued, the text naming the clip at fault: null pointers; B < 0; a clip shorter
 * than n_fft; a negative offset; two clips that overlap; an output whose extent (first clip .. last clip) overlaps the audio's, the
 * workspace or the other output; a workspace off a 16-byte boundary; a capturing stream (the tables come from a staging buffer);
 * the configurations smh_hpss_resynth_f32 refuses.  B == 0 returns SMH_OK and touches nothing.  Every offset is 64-bit. */
int smh_hpss_audio_ragged_sizes(const smh_ctx *ctx, const long long *h_offsets, const int *h_lengths, int B, int *h_T /* or NULL */,
                                size_t *work_bytes /* or NULL */);
int smh_hpss_audio_ragged_f32(const smh_ctx *ctx, const float *d_audio, const long long *h_offsets, const int *h_lengths, int B,
                              float *d_y_harm, float *d_y_perc, void *d_work, size_t work_bytes, void *stream);

/* ---- a4: librosa.feature.melspectrogram(S=X, n_mels=) = mel_basis(22050, n_fft) @ X ---------
 * d_X (B, K, T) -> d_Y (B, n_mels, T)  (preprocessing.py:409-410,419,421)                       */
int smh_mel_f32(const smh_ctx *ctx, const float *d_X, int B, int T, float *d_Y, void *stream);

/* ---- a5: librosa.core.power_to_db(X**2): 10*log10(max(1e-10, x^2)), then max(., max-80) with the
 * max taken over each of the `n_arrays` arrays of `elems` values (preprocessing.py:420,422)      */
int smh_power_to_db_sq_f32(const smh_ctx *ctx, const float *d_X, int n_arrays, int elems, float *d_Y, void *stream);

/* ---- a7(iii): StandardScaler per row over frames (preprocessing.py:211-214,221-224) ----------
 * d_X (n_rows, T) -> d_Y (n_rows, T): (x-mean)/std, population std, std==0 -> 1                  */
int smh_standardize_rows_f32(const smh_ctx *ctx, const float *d_X, int n_rows, int T, float *d_Y, void *stream);

/* ---- a8: tools.extract_patches incl. the tile-if-short rule of get_feature_patches -----------
 * d_FV (B, F, T) -> patches.  layout 0: (B*nP, F, W) as the reference returns; layout 1:
 * (B*nP, W, F) time-major = the TCN input after np.transpose (Proposed_Work_Results.py:235-236).
 * Frames are taken modulo T when T < W (the tiled featuregram).  Returns nP per clip (>=0).     */
int smh_extract_patches_f32(const smh_ctx *ctx, const float *d_FV, int B, int F, int T, int W, int shift, int layout,
                            float *d_out, void *stream);

/* Layouts of the harmonic median between smh_hpss_median_ex_f32 and the feature stage (harm_layout):
 *   0 = (B, K, T) as the reference returns it, 1 = (B, T, K), 2 = (B, ceil(T/16), K, 16) -- 16-frame blocks, written
 *   by the block-split median kernels (windows <= 21; any clip length, tile by tile) and read by the single-kernel feature
 *   path.  A harm buffer of smh_harm_buffer_floats(K, T) floats per clip has room for every layout;
 *   smh_features_blocked_ok tells whether the feature stage accepts layout 2 for clips of T frames (with_l0: together
 *   with the layer-0 fusion of smh_features_l0_f32).  smh_hpss_median_ex_f32 returns the layout it actually wrote.  */
size_t smh_harm_buffer_floats(int K, int T);
int smh_features_blocked_ok(const smh_ctx *ctx, int T, int with_l0);

/* ---- a3..a9 in two launches: (S, harm, perc) -> featuregram -> standardised time-major patches ------
 * soft masks + mel + power_to_db (preprocessing.py:418-424) then tile / StandardScaler / patches /
 * transpose (preprocessing.py:137-142,208-234; Proposed_Work_Results.py:235-236).
 * d_fv (B, 2*rows, T) out; d_patches (B*nP, W, 2*rows) out or NULL; d_maxkeys: 2*B int32 scratch.
 * Returns nP per clip.                                                                            */
int smh_features_f32(const smh_ctx *ctx, const float *d_S, const float *d_harm, const float *d_perc, int B, int T,
                     int W, int shift, float *d_fv, float *d_patches, int32_t *d_maxkeys, void *stream);
/* same, with d_harm in the layout returned by smh_hpss_median_ex_f32 */
int smh_features_ex_f32(const smh_ctx *ctx, const float *d_S, const float *d_harm, const float *d_perc, int harm_layout,
                        int B, int T, int W, int shift, float *d_fv, float *d_patches, int32_t *d_maxkeys, void *stream);

/* ---- patch layout of the harmonic-percussive front end (patch_layout), numbered like smh_extract_patches_f32's `layout`:
 *   0 = image (B*nP, 2*rows, W), frame index fastest, harmonic rows first: what get_feature_patches returns
 *       (np.append(patches_H, patches_P, axis=1), lib/preprocessing.py:201-234) -- the Conv2D models' input before
 *       np.expand_dims(.., axis=3);
 *   1 = time-major (B*nP, W, 2*rows): the TCN's input after the Lemaire-only transpose (Proposed_Work_Results.py:235-236).
 * A patch value is the same f32 number in either layout; only its address differs, and the featuregram is the same bits.  The
 * finishing kernels write the asked-for layout directly (no transpose pass).  smh_features_layout_f32, smh_frontend_layout_f32 and
 * smh_frontend_ragged_layout_f32 are smh_features_ex_f32, smh_frontend_f32 and smh_frontend_ragged_f32 with that one argument
 * more; the old entries call them with 1.  Any other value returns SMH_E_INVALID (text in smh_last_error) before any launch.
 * smh_frontend_ragged_sizes serves both: h_patch_off counts patches, and a patch is W * 2*rows floats in either layout.
 * (The layer-0 entry smh_features_l0_f32 writes time-major patches only; the plain front end has layout entries of its own below.) */
int smh_features_layout_f32(const smh_ctx *ctx, const float *d_S, const float *d_harm, const float *d_perc, int harm_layout,
                            int B, int T, int W, int shift, int patch_layout, float *d_fv, float *d_patches,
                            int32_t *d_maxkeys, void *stream);
int smh_frontend_layout_f32(const smh_ctx *ctx, const float *d_audio, int B, int n_samples, int W, int shift, int patch_layout,
                            float *d_fv, float *d_patches, void *d_work, size_t work_bytes, float *d_S, float *d_harm,
                            float *d_perc, void *stream);
int smh_frontend_ragged_layout_f32(const smh_ctx *ctx, const float *d_audio, const long long *h_offsets, const int *h_lengths,
                                   int B, int W, int shift, int patch_layout, float *d_fv, float *d_patches /* or NULL */,
                                   void *d_work, size_t work_bytes, void *stream);

/* ---- fused fast path: get_featuregram (from Xin) + get_feature_patches for a batch of clips ---
 * d_audio (B, n_samples) -> d_fv (B, 2*rows, T)  [the featuregram, = get_featuregram's return]
 *                        -> d_patches (B*nP, W, 2*rows) time-major, standardised  [may be NULL]
 * d_work: smh_frontend_workspace_bytes() bytes of scratch.  Optional parity taps (may be NULL):
 * d_S, d_harm, d_perc (B, K, T).  Returns nP per clip.                                          */
size_t smh_frontend_workspace_bytes(const smh_ctx *ctx, int B, int n_samples);
int smh_frontend_f32(const smh_ctx *ctx, const float *d_audio, int B, int n_samples, int W, int shift, float *d_fv,
                     float *d_patches, void *d_work, size_t work_bytes, float *d_S, float *d_harm, float *d_perc,
                     void *stream);

/* ---- ragged batches: B clips of DIFFERENT lengths in one call (the reference's generators take whole files of any length
 * one at a time: Proposed_Work_Results.py:92-95, 131-134, 189-192, 465-474).  d_audio holds the clips at sample offsets
 * h_offsets[b] with h_lengths[b] samples each (HOST arrays; keep every offset a multiple of 4 samples = 16 bytes: a clip that
 * starts off an 8-byte boundary is processed alone, through smh_frontend_f32).  ONE LAUNCH PER STAGE for all clips: the lengths
 * become a descriptor table + (clip, tile) work lists, uploaded in one copy from a pinned slot of the context, and the STFT, the
 * medians and the feature kernels each run once over every clip (smh_ragged.hip); a clip gets bit for bit what smh_frontend_f32
 * gives it alone or in an equal-length batch.  Outputs are concatenated: clip b's featuregram (2*rows, T_b) starts at float
 * h_fv_off[b] of d_fv, its nP_b standardised time-major patches at patch h_patch_off[b] of d_patches ((W, 2*rows) each).
 * smh_frontend_ragged_sizes fills the per-clip tables (each may be NULL) and the workspace requirement (tables + S / harm / perc of
 * every clip, at most 8 GiB: beyond that, or with a smaller workspace than asked for, the call runs in sub-batches; never less than
 * the largest single clip needs); W <= 0: no patches.  d_work must start on a 16-byte boundary.  Stream-ordered on `stream`; not
 * capturable in a hipGraph (the table upload reads a staging buffer that the next call rewrites). */
int smh_frontend_ragged_sizes(const smh_ctx *ctx, const long long *h_offsets, const int *h_lengths, int B, int W, int shift,
                              long long *h_fv_off /* B+1 */, long long *h_patch_off /* B+1 */, int *h_T /* B */,
                              int *h_nP /* B */, size_t *work_bytes);
int smh_frontend_ragged_f32(const smh_ctx *ctx, const float *d_audio, const long long *h_offsets, const int *h_lengths, int B,
                            int W, int shift, float *d_fv, float *d_patches /* or NULL */, void *d_work, size_t work_bytes,
                            void *stream);

/* ---- the four feature branches WITHOUT harmonic-percussive separation (lib/preprocessing.py:378-402): Spec, LogSpec, MelSpec,
 * LogMelSpec.  One featuregram of `rows` = smh_ctx_feat_rows() rows per clip (no H || P pair), no medians, no soft masks:
 *     n_mels <= 0, log_db = 0   Spec        fv = |S|
 *     n_mels <= 0, log_db = 1   LogSpec     fv = power_to_db(|S|**2)
 *     n_mels >  0, log_db = 0   MelSpec     fv = mel @ |S|**2                  (melspectrogram(y=..., sr=fs): power = 2.0)
 *     n_mels >  0, log_db = 1   LogMelSpec  fv = power_to_db((mel @ |S|**2)**2)
 * The mel branches project the POWER spectrogram, and the reference builds their basis for sr = fs: create the context with
 * mel_sr = fs (16000), not the 22050 of the '*HarmPerc*' branches.  power_to_db: ref 1, amin 1e-10 on the f32 square, top_db 80 below
 * the maximum of the clip's whole array.  Read from the context: n_fft, win_length, hop, n_mels, log_db, mel_sr and the STFT
 * precision; l_harm and l_perc are ignored.  The mel projection keeps a K x 64-frame image in LDS: n_fft <= 1198 with a filterbank.
 * Any T >= 1 takes the same two kernels (smh_plain.hip), so a clip gets the same bits alone, in a batch and in a ragged call.
 *
 * smh_plain_features_f32: d_S (B, K, T) -> d_fv (B, rows, T) and, with d_patches, the standardised time-major patches
 *   (B*nP, W, rows) of get_feature_patches (tile-if-short, StandardScaler per row over the frames, tools.extract_patches, transpose).
 *   d_maxkeys: B int32 of scratch.  Returns nP per clip.
 * smh_plain_frontend_f32: d_audio (B, n_samples) -> the same, through the context's STFT; d_work of
 *   smh_plain_frontend_workspace_bytes() bytes; d_S (B, K, T): optional tap of the magnitude spectrogram, or NULL.
 * smh_plain_frontend_ragged_sizes / _f32: the contract of smh_frontend_ragged_sizes / smh_frontend_ragged_f32 above -- host offset and
 *   length tables, one launch per stage over all clips, concatenated outputs, sub-batches when the workspace is smaller than asked
 *   for -- with h_fv_off counting rows * T_b floats per clip and patches of (W, rows) floats.
 * smh_plain_features_layout_f32 / smh_plain_frontend_layout_f32 / smh_plain_frontend_ragged_layout_f32: the three entries above with
 *   one argument more, patch_layout, numbered as for the harmonic-percussive entries: 0 = image (B*nP, rows, W), frame index fastest,
 *   what get_feature_patches returns and the single-task Conv2D baselines read before np.expand_dims(.., axis=3); 1 = time-major
 *   (B*nP, W, rows).  The same f32 values at other addresses, written by the finishing kernel itself (no transpose pass); the
 *   featuregram is the same bits.  The old entries call these with 1.  smh_plain_frontend_ragged_sizes serves both: a patch is
 *   W * rows floats in either layout.  Any other patch_layout is SMH_E_INVALID before any launch.
 * Bad arguments return SMH_E_INVALID (text in smh_last_error) before any launch. */
int smh_plain_features_f32(const smh_ctx *ctx, const float *d_S, int B, int T, int W, int shift, float *d_fv,
                           float *d_patches /* or NULL */, int32_t *d_maxkeys /* B */, void *stream);
size_t smh_plain_frontend_workspace_bytes(const smh_ctx *ctx, int B, int n_samples);
int smh_plain_frontend_f32(const smh_ctx *ctx, const float *d_audio, int B, int n_samples, int W, int shift, float *d_fv,
                           float *d_patches /* or NULL */, void *d_work, size_t work_bytes, float *d_S /* or NULL */, void *stream);
int smh_plain_frontend_ragged_sizes(const smh_ctx *ctx, const long long *h_offsets, const int *h_lengths, int B, int W, int shift,
                                    long long *h_fv_off /* B+1 */, long long *h_patch_off /* B+1 */, int *h_T /* B */,
                                    int *h_nP /* B */, size_t *work_bytes);
int smh_plain_frontend_ragged_f32(const smh_ctx *ctx, const float *d_audio, const long long *h_offsets, const int *h_lengths, int B,
                                  int W, int shift, float *d_fv, float *d_patches /* or NULL */, void *d_work, size_t work_bytes,
                                  void *stream);
int smh_plain_features_layout_f32(const smh_ctx *ctx, const float *d_S, int B, int T, int W, int shift, int patch_layout, float *d_fv,
                                  float *d_patches /* or NULL */, int32_t *d_maxkeys /* B */, void *stream);
int smh_plain_frontend_layout_f32(const smh_ctx *ctx, const float *d_audio, int B, int n_samples, int W, int shift, int patch_layout,
                                  float *d_fv, float *d_patches /* or NULL */, void *d_work, size_t work_bytes,
                                  float *d_S /* or NULL */, void *stream);
int smh_plain_frontend_ragged_layout_f32(const smh_ctx *ctx, const float *d_audio, const long long *h_offsets, const int *h_lengths,
                                         int B, int W, int shift, int patch_layout, float *d_fv, float *d_patches /* or NULL */,
                                         void *d_work, size_t work_bytes, void *stream);

/* ---- 8f rank 1: load_and_preprocess_signal after the decode (lib/preprocessing.py:330-350) ------------------
 * Batched over B clips of N samples each, resident on the device.  Floating point: the mean is accumulated in
 * f64 in a fixed order (numpy: pairwise f32), everything else is the same f32 arithmetic as numpy.           */
/* bytes of device workspace for smh_normalize_f32 / for the silence functions (hop = frame shift in samples) */
size_t smh_normalize_workspace_bytes(int B, int N);
size_t smh_silence_workspace_bytes(int B, int N, int hop);
/* Xin -= mean(Xin); Xin /= max|Xin| per clip (preprocessing.py:332-333,348-349).  d_out may alias d_x.        */
int smh_normalize_f32(const float *d_x, int B, int N, float *d_out, void *d_work, size_t work_bytes, void *stream);
/* librosa.feature.rms(y=, frame_length=, hop_length=)[0] (preprocessing.py:338): center=True, reflect padding.
 * d_y (B, N) -> d_energy (B, nFrames); returns nFrames = 1 + (N + 2*(frame_length/2) - frame_length)/hop.      */
int smh_rms_f32(const float *d_y, int B, int N, int frame_length, int hop, float *d_energy, void *stream);
/* tools.removeSilence(Xin, nSamples, energy, nFrames, fs, Tw, Ts, alpha, beta) (lib/cython_impl/tools.pyx:42-134),
 * integer-exact given the energies: float threshold alpha*max(energy), scipy medfilt(marker, 5) with zero padding,
 * the literal run loop, removal only when at least two runs exceed beta seconds.  d_out (B, N) keeps the input
 * length: retained samples first, then the reference's tail of 1.0 (unchanged copy when nothing is removed).
 * Optional outputs (null to skip): d_sample_marker (B, N) u8, d_frame_marker (B, nFrames) i32, d_n_keep (B) i32 =
 * number of retained samples (N when nothing was removed).  d_out must not alias d_x.                         */
int smh_remove_silence_f32(const float *d_x, int B, int N, const float *d_energy, int nFrames, int fs, int Tw, int Ts,
                           double alpha, double beta, float *d_out, unsigned char *d_sample_marker, int *d_frame_marker,
                           int *d_n_keep, void *d_work, size_t work_bytes, void *stream);
/* preprocessing.py:332-349 in one call: normalise, rms(frameSize, frameShift), removeSilence (alpha=0.025,
 * beta=0.075), normalise again (tail of ones included, as in the reference).  The "< 0.1 s: duplicate" rule of
 * :343-346 depends on N alone and stays with the host caller.                                                  */
int smh_preprocess_signal_f32(const float *d_x, int B, int N, int fs, int Tw, int Ts, float *d_out, int *d_n_keep,
                              void *d_work, size_t work_bytes, void *stream);

/* ---- 8f rank 2: mix_signals(Xin_sp, Xin_mu, target_dB) (lib/preprocessing.py:297-325) for B pairs of clips ------
 * d_sp (B, N) speech, d_mu (B, N_mu) music (looped to N when shorter, cut when longer), d_target_db (B) SMR in dB ->
 * d_out (B, N): music scaled to the target speech-to-music ratio, both weighted so the factors sum to one, then the
 * reference's normalisation.  Energies are f64 ordered sums (numpy: pairwise f32).  Workspace:
 * smh_normalize_workspace_bytes(B, N).                                                                          */
int smh_mix_signals_f32(const float *d_sp, const float *d_mu, int B, int N, int N_mu, const float *d_target_db,
                        float *d_out, void *d_work, size_t work_bytes, void *stream);

/* ---- 8f rank 4: scipy.signal.medfilt(x, kernel_size) on B tracks of n values (zero padded, odd window <= 8191),
 * the smoothing of the frame-level probability track (DAFx12_Speech_Music_Detection_B3_MTL_v2.py:94-98, window 501).
 * Bit-exact selection.  d_y must not alias d_x.                                                                 */
int smh_medfilt1d_f32(const float *d_x, int B, int n, int kernel_size, float *d_y, void *stream);

/* ---- the other two functions of lib/cython_impl/tools.pyx (off by default on the hot path), float64 like the reference:
 * scale_data(FV, mean, stdev) :138-165 -> (FV - mean[f]) / (stdev[f] + 1e-10), FV (F, T);
 * get_data_statistics(FV, stat_type, axis) :169-215 for patches (N, F, T): stat 0 mean, 1 variance (population),
 * 2 skew, 3 kurtosis (scipy.stats, biased, Fisher); axis 0 reduces over the rows -> (N, T), axis 1 over the frames ->
 * (N, F).                                                                                                            */
int smh_scale_data_f64(const double *d_FV, int F, int T, const double *d_mean, const double *d_stdev, double *d_out,
                       void *stream);
int smh_data_statistics_f64(const double *d_FV, int N, int F, int T, int stat, int axis, double *d_out, void *stream);

/* ---- frame-level scaling on the device path (PARAMS['frame_level_scaling']): the moments get_data_stats needs
 * (lib/preprocessing.py:461-586) and scale_data + extract_patches in one kernel.  Both work on B featuregrams that are already
 * on the device: h_fv[b] is the DEVICE pointer of featuregram b, (rows, h_T[b]) float32, dense (rows of exactly h_T[b] floats),
 * h_T[b] >= 1; h_fv and h_T themselves are host arrays.  The featuregrams may be separate allocations or views of one buffer.
 * The per-clip table is uploaded through a staging slot of ctx (any front-end context; its configuration is not read), so the
 * calls cannot be captured in a graph; more clips than one slot holds are split into several launches.
 *
 * smh_row_moments_f64: d_moments (B, rows, 2) float64 = {sum(x), M2 = sum((x - sum(x) / T)^2)} of every (clip, row), d_nonfinite
 * (B, rows) int32 = how many of the row's values are NaN or +-inf (its moments are then not finite).  One f64 partial sum per
 * lane over the frames lane, lane + 64, ... and a fixed xor tree over the 64 lanes: the summation order depends on T alone, so a
 * clip's moments are bit-identical alone and in any batch.  Around any mean mu, sum((x - mu)^2) = M2 + T (sum(x) / T - mu)^2.
 *
 * smh_scaled_patches_f32: every patch element is (float)(((double)x - d_mean[r]) / (d_stdev[r] + 1e-10)) -- scale_data's float64
 * arithmetic (tools.pyx:157-164) rounded once to float32 -- on the grid of smh_tiled_frames / smh_num_patches / smh_patch_start
 * (T < W: tiled-if-short).  d_mean, d_stdev: (rows) float64 on the device.  Clip b's patches follow those of the clips before it:
 * d_patches is (sum_b nP_b, W, rows) with patch_layout 1 (time-major) or (sum_b nP_b, rows, W) with 0 (image), where nP_b =
 * smh_num_patches(smh_tiled_frames(h_T[b], W), W, shift); smh_scaled_patches_count returns the sum (< 0 on error) and, if
 * h_patch_off is not null, the B + 1 running sums.                                                                       */
int smh_row_moments_f64(const smh_ctx *ctx, const float *const *h_fv, const int *h_T, int B, int rows, double *d_moments,
                        int32_t *d_nonfinite, void *stream);
long long smh_scaled_patches_count(const int *h_T, int B, int W, int shift, long long *h_patch_off);
int smh_scaled_patches_f32(const smh_ctx *ctx, const float *const *h_fv, const int *h_T, int B, int rows, const double *d_mean,
                           const double *d_stdev, int W, int shift, int patch_layout, float *d_patches, void *stream);

/* ---- the skewness-vector feed (PARAMS['skewness_vector'] = 'Row' / 'Col'): get_data_statistics of every patch, taken straight
 * from featuregrams on the device -- h_fv, h_T, B, rows, W, shift, the per-clip table and the patch grid exactly as for
 * smh_scaled_patches_f32 (patch counts and offsets: smh_scaled_patches_count); no patch is written.  stat: 0 mean, 1 variance,
 * 2 skew, 3 kurtosis as smh_data_statistics_f64 numbers them.  axis 1 reduces over the W frames of a patch: d_out is
 * (sum_b nP_b, rows); axis 0 over the rows of a frame: (sum_b nP_b, W).  d_out is float64 (out_f32 = 0) or float32 rounded once from
 * the float64 result.  The value under the statistic is the patch element the existing entries write, bit for bit: with d_mean =
 * d_stdev = NULL smh_standardize_rows_f32's per-file StandardScaler value (statistics over the file's own h_T[b] frames), with both
 * given ((rows) float64 on the device) smh_scaled_patches_f32's.  The statistic is float64 and two-pass (the mean, then the central
 * moments of x - mean, sums in index order); a window with m2 == 0 has skew 0 and kurtosis -3.  The order of every addition depends
 * on W (axis 1) or rows (axis 0) alone: a file's vectors are bit-identical alone and in any batch.  A clip without a patch writes
 * nothing.  axis 1 takes W <= 8192.  d_work: smh_patch_statistics_workspace_bytes(B, rows, axis, with_stats) bytes, 8-byte aligned
 * (0 bytes, and d_work may be NULL, for axis 1 or with statistics).                                                               */
size_t smh_patch_statistics_workspace_bytes(int B, int rows, int axis, int with_stats);
int smh_patch_statistics(const smh_ctx *ctx, const float *const *h_fv, const int *h_T, int B, int rows, const double *d_mean,
                         const double *d_stdev, int W, int shift, int stat, int axis, int out_f32, void *d_out, void *d_work,
                         size_t work_bytes, void *stream);

/* ---- a10-a12: B3_MTL = get_Lemaire_MTL_model (lib/proposed_architectures.py:85-170, 25-80) ---- */
typedef struct smh_model_cfg {
    int32_t n_feat;     /* N_MELS argument = input_shape[1]: 240                       */
    int32_t patch_size; /* W: 68 / 99 / 249                                            */
    int32_t n_classes;  /* 3 (heads S,M,R[2],3C) or 5 (heads S,M,N,R[3],3C)            */
    int32_t nb_filters; /* 32                                                          */
    int32_t kernel_size;/* 3                                                           */
    int32_t nb_stacks;  /* 3                                                           */
    int32_t n_dilations;/* 8 -> dilations 1,2,...,128                                  */
    int32_t block_variant; /* residual block of the third-party `tcn.TCN` (lib/proposed_architectures.py:124-144), which the
                            * reference does not pin: 0 = keras-tcn 2.3.x (initial 1x1 conv; per block dilated conv -> relu ->
                            * channel-max normalisation ('norm_relu') -> dropout -> 1x1 conv -> + input; final relu) -- the API
                            * the reference's positional call binds under, the default, training and the fused bench path;
                            * 1 = keras-tcn >= 2.8 (no initial conv; per block two dilated convs, relu each, shortcut = input or
                            * a 1x1 'matching' conv, relu of the sum) -- inference forward only (smh_model_forward_f32).
                            * Canonical weight order for 1: per block [conv0 kernel (3,Cin,32), bias, conv1 kernel (3,32,32),
                            * bias, (first block, unless n_feat == 32: matching kernel (1,n_feat,32), bias)], then '3C' and the
                            * heads as for 0.  n_feat == 32: the channel counts agree, identity shortcut in every block. */
} smh_model_cfg;
#define SMH_TCN_BLOCK_2_3 0
#define SMH_TCN_BLOCK_2_8 1

int smh_model_create(const smh_model_cfg *cfg, smh_model **out);
/* Head kind of the model.  SMH_HEADS_MTL: the independent heads of MTL_modifications (lib/proposed_architectures.py:25-80) -- what
 * smh_model_create builds.  SMH_HEADS_CASCADED: get_Lemaire_Cascaded_MTL_model (:175-323): the same trunk, '3C' and Dense(16) layers;
 * R = Dense(2)(Dropout(relu(BN(Dense16)))); S and M = sigmoid(Dense(1)(BN18(concat[Dropout(relu(BN(Dense16))), R]))).  Heads are
 * always S, M, R[2] (n_classes widens '3C' only), so out_dim = 4 + n_classes.  Canonical order as for SMH_HEADS_MTL except that S and
 * M carry, between their moving_variance and out kernel, the concatenation BatchNorm [gamma, beta, moving_mean, moving_variance]
 * (18 each) and an out kernel of shape (18, 1).  The bf16 forwards and trainer dtype 1 refuse a cascaded model. */
#define SMH_HEADS_MTL 0
#define SMH_HEADS_CASCADED 1
/* SMH_HEADS_FUSION: get_Lemaire_MTL_intermediate_fusion_model (:327-420): two inputs harm_input / perc_input, each (N, W, n_feat)
 * with cfg.n_feat the PER-BRANCH width, two independent TCN trunks 'tcn_initial_conv_H' / '_P', x = BatchNorm(concat[Flatten(trunk
 * H), Flatten(trunk P)]) over D = 2 * W * 32 features (moving statistics, eps 1e-3), then B3_MTL's '3C' and heads on x.  out_dim as
 * for SMH_HEADS_MTL.  Canonical order: trunk H [initial_conv kernel (1, n_feat, 32), bias, per block conv kernel, bias, conv1x1
 * kernel, bias], trunk P (the same), the fused BatchNorm [gamma, beta, moving_mean, moving_variance] (D each), '3C' kernel (D,
 * n_classes), bias, then per head [dense kernel (D, 16), bias, gamma, beta, moving_mean, moving_variance, out kernel, out bias].
 * Only the two-input entry points below serve it: every single-input forward, smh_train_step_f32, the bf16 forwards, trainer
 * dtype 1 and block_variant 1 refuse a fusion model. */
#define SMH_HEADS_FUSION 2
/* SMH_HEADS_SINGLE: the single-task Lemaire TCN baseline, get_Lemaire_model (lib/baseline_architectures.py:196-300; 5-class twin:
 * 5_class_classification.py:54-145): B3_MTL's trunk, then Flatten -> Dense(n_classes) -> softmax.  No heads (n_heads = 0), n_classes
 * 2, 3 or 5, out_dim = n_classes: a row of d_out is the softmax alone.  Canonical order: the trunk exactly as for SMH_HEADS_MTL, then
 * 'dense' kernel (patch_size * 32, n_classes), bias.  Served by smh_model_forward_f32 (with the d_trunk tap),
 * smh_model_forward_dense_f32, smh_model_eval_losses_f32 (d_sums = [total | loss | accuracy]) and the f32 trainer:
 *   n_classes == 2: Keras' binary_crossentropy on the two softmax outputs (clipped to [1e-7, 1 - 1e-7], + 1e-7 inside the logs, mean
 *     over the two outputs, then over the batch) and BINARY accuracy, the mean over all N x 2 outputs of (p > 0.5) == y;
 *   n_classes 3 / 5: categorical cross-entropy and categorical accuracy.
 * smh_train_step_f32: d_y (N, n_classes) one-hot, d_drop_heads ignored, h_loss_weights one float or NULL, d_losses four floats
 * [loss, weighted loss, accuracy, 0].  The trainer's bucket is the gradient alone (no BatchNorm statistics): smh_model_num_params
 * floats.  smh_model_forward_x0_* (the plain front end writes no layer-0 partials), the bf16 forwards, trainer dtype 1, block_variant
 * 1, the fusion entries and smh_late_fusion_create refuse a single-task model. */
#define SMH_HEADS_SINGLE 3
int smh_model_create_heads(const smh_model_cfg *cfg, int heads, smh_model **out);
void smh_model_destroy(smh_model *m);
/* number of float32 parameters in canonical (Keras-layout) order, see DESIGN.md "weight order" */
size_t smh_model_num_params(const smh_model *m);
/* upload weights given as ONE flat host float32 array in canonical order */
int smh_model_set_weights(smh_model *m, const float *h_flat, size_t n, void *stream);
/* total width of the concatenated head outputs per patch: 3-class: 1+1+2+3 = 7; 5-class: 11 */
int smh_model_out_dim(const smh_model *m);
/* inference forward.  d_x (N, W, n_feat) float32 time-major -> d_out (N, out_dim) float32 holding
 * [S | M | (N) | R | 3C-softmax] per row, i.e. model.predict's list concatenated on axis 1
 * (Proposed_Work_Results.py:520,586).  d_trunk (N, W, nb_filters) optional TCN output tap.      */
int smh_model_forward_f32(const smh_model *m, const float *d_x, int N, float *d_out, float *d_trunk, void *stream);
/* Error contract of the stream-ordered forwards (SURVEY 8(b) "Errors": the reference raises; a launch cannot).  Every
 * smh_model_forward_* (and the training forward inside smh_train_step_f32) only enqueues work, so a condition a kernel meets on the
 * device -- today one: a wave whose dependency (a tile flag of the barrier-free block schedule, the partner half of a split tile of
 * the barrier schedule) did not arrive within its bounded spin -- is recorded in the model's device error word; the affected
 * outputs are NOT results (zero-filled by the barrier-free schedule, computed from a stale exchange by the split tile).
 * smh_model_status waits for `stream`, returns SMH_OK or SMH_E_DEVICE (+ smh_last_error) and clears the word.  The Python side calls
 * it wherever results leave the device or decide something: `predict`, the device `evaluate`, `patch_probabilities`, `train_on_batch`
 * (sync=True) and once per epoch in `fit`. */
int smh_model_status(smh_model *m, void *stream);

/* download the (device-resident, possibly trained) weights in canonical order */
/* Fusion of the network's first layer into the feature stage (bench fast path; same logits within f32 tolerance):
 * smh_features_l0_f32 = smh_features_ex_f32 that also emits, per clip half, its share of B3_MTL's initial Conv1D(32, 1)
 * on the standardised patches, d_x0p (B*nP, 2, W, 32) float32, from the canonical kernel d_w0 = smh_model_w0_ptr(model)
 * ((n_feat, 32), n_feat = 2 * feat_rows); d_patches may be null.  smh_model_forward_x0_f32 = smh_model_forward_f32
 * that starts from those partials (adds them and the bias) instead of reading (N, W, n_feat) patches.              */
const float *smh_model_w0_ptr(const smh_model *m);
int smh_features_l0_f32(const smh_ctx *ctx, const float *d_S, const float *d_harm, const float *d_perc, int harm_layout,
                        int B, int T, int W, int shift, float *d_fv, float *d_patches, const float *d_w0, float *d_x0p,
                        int32_t *d_maxkeys, void *stream);
int smh_model_forward_x0_f32(const smh_model *m, const float *d_x0p, int N, float *d_out, float *d_trunk, void *stream);
/* model.evaluate's arithmetic for one batch (Proposed_Work_Results.py:160-165 losses, 683-687 evaluate): from d_out (N, out_dim) as
 * smh_model_forward_f32 wrote it and d_targets (N, out_dim) in the same column order [S | M | (N) | R | 3C], the batch means of the
 * inference-mode losses -- binary cross-entropy on the sigmoid heads, mean squared error on 'R', categorical cross-entropy on '3C', all
 * with Keras' 1e-7 clipping, float64 arithmetic --, the '3C' accuracy and the total loss sum_i h_loss_weights[i] * loss_i + l2_penalty
 * (h_loss_weights: n_heads + 1 host doubles in output order; l2_penalty: the heads' kernel-regulariser term, a function of the weights
 * only), each multiplied by `weight` and ADDED to d_sums[n_heads + 3] = [total | head losses in output order | 3C loss | 3C accuracy]
 * (float64, zeroed by the caller): a validation pass accumulates on the device and reads back once. */
int smh_model_eval_losses_f32(const smh_model *m, const float *d_out, const float *d_targets, int N, double weight,
                              const double *h_loss_weights, double l2_penalty, double *d_sums, void *stream);
/* Dense file-level inference: the per-batch body of `patch_probability_generator`,
 * DAFx12_Speech_Music_Detection_B3_MTL_v2.py:634-665 -- every hop-`shift` patch of a 10 000-frame batch of one file's featuregram
 * through model.predict.  d_fv (n_feat, Tc) float32: the batch as get_feature_patches leaves it in front of the patch extraction
 * (each half standardised over the batch, lib/preprocessing.py:208-224); patch p = frames [min(p*shift, Tc - W), + W), p <
 * smh_num_patches(Tc, W, shift) -- tools.extract_patches' grid (tools.pyx:24-34).  Returns the number of patches (>= 0) or an error;
 * d_out (nP, out_dim) as smh_model_forward_f32 writes it, to the same f32 tolerance.  Nothing of size nP x W x n_feat is built: the
 * first layer (a 1x1 convolution) is evaluated once per FRAME into d_work ((2, Tc, 32) float32 =
 * smh_model_dense_workspace_bytes) and every patch is read as a window of it.  Needs Tc >= W (shorter batches are tiled by
 * get_feature_patches: build the patches and call smh_model_forward_f32), n_feat a multiple of 8, block_variant 0.
 * On return (once the stream has run) d_work holds the per-frame layer-0 partials (2, Tc, 32) float32, laid out
 * [half][frame][channel]: half h is the product of rows [h * n_feat / 2, + n_feat / 2) of d_fv with the same rows of the layer-0
 * kernel, WITHOUT the layer-0 bias.  Both dense entries leave the same bits there. */
size_t smh_model_dense_workspace_bytes(const smh_model *m, int Tc);
int smh_model_forward_dense_f32(const smh_model *m, const float *d_fv, int Tc, int shift, void *d_work, size_t work_bytes,
                                float *d_out, void *stream);
/* Same forward with bf16 matrix-core operands and f32 accumulation / residual stream / normalisation (BASELINE config 5,
 * "mixed bf16 CNN + fp32 HPSS").  Weights are split once per weight version, activations right before each product.
 *   split = 1 (what smh_model_forward_bf16 runs): every operand is hi + lo (two bf16 values, 16 mantissa bits), every
 *     product is hi*hi + hi*lo + lo*hi on v_mfma_f32_16x16x32_bf16 -- three bf16 products per f32 product, still 5x fewer
 *     matrix-core cycles than the exact-f32 MFMA.  Outputs within 2e-2 of smh_model_forward_f32 (tests state the measured
 *     distance, ~1e-3), which SURVEY 8(d') asks of a bf16 variant.
 *   split = 0: operands rounded to one bf16.  Faster again, but 24 blocks of "divide by the channel maximum" amplify the
 *     8-bit operand rounding to 3.5-5e-2 at the outputs: outside the tolerance, kept for measurement only.
 * Neither is the parity path: smh_model_forward_f32 is. */
int smh_model_forward_bf16(smh_model *m, const float *d_x, int N, float *d_out, void *stream);
int smh_model_forward_bf16_ex(smh_model *m, const float *d_x, int N, float *d_out, int split, void *stream);
/* The same from the layer-0 partials of smh_features_l0_f32 (the bench fast path; layer 0 is then exact f32): d_x0p
 * (N, 2, patch_size, 32) float32 as for smh_model_forward_x0_f32. */
int smh_model_forward_x0_bf16(smh_model *m, const float *d_x0p, int N, float *d_out, int split, void *stream);
/* Dense file-level inference on split bf16 operands (always split = 1; the B3_MTL heads and block_variant 0 only, as
 * smh_model_forward_bf16): the arguments, the return value (the number of patches >= 0, or an error), the checks and the workspace
 * (smh_model_dense_workspace_bytes) of smh_model_forward_dense_f32.  Layer 0 stays exact f32: the same per-frame pass writes the
 * same partials (2, Tc, 32), [half][frame][channel] without the layer-0 bias, into d_work, and the split-operand network reads
 * every patch as a window of them -- bit for bit what smh_model_forward_x0_bf16 computes on the same windows gathered into
 * (nP, 2, patch_size, 32).  The split operand cache follows the weight version as in smh_model_forward_bf16. */
int smh_model_forward_dense_bf16(smh_model *m, const float *d_fv, int Tc, int shift, void *d_work, size_t work_bytes, float *d_out,
                                 void *stream);
int smh_model_get_weights(const smh_model *m, float *h_flat, size_t n, void *stream);

/* ---- a13: Conv2D MTL baselines, inference forward (lib/proposed_architectures.py:425-511 Doukhan, :516-588
 * Papakostas, :650-764 Jang; heads :25-80).  Input: (N, in_h, in_w) float32 images = the (nP, 2F, W, 1) patches of
 * get_feature_patches for the non-Lemaire models (lib/preprocessing.py:216-217,226-227).  Output row =
 * [S | M | (N) | R | 3C], like smh_model_forward_f32.  Weights: one flat float32 vector, tensors in the order
 * reported by smh_cnn_tensor_info (Keras layouts: Conv2D (kh,kw,Cin,Cout), Dense (in,out), BN gamma/beta/mean/var). */
enum { SMH_CNN_DOUKHAN = 0, SMH_CNN_PAPAKOSTAS = 1, SMH_CNN_JANG = 2,
       /* the single-task baselines of lib/baseline_architectures.py (get_Doukhan_model :62-108, get_Papakostas_model :147-175,
        * get_Jang_model :358-442): no S / M / R heads (n_heads = 0), n_classes 2 or 3, out_dim = n_classes -- a row of d_out is the
        * softmax alone.  The last tensors are 'dense/kernel' (D, n_classes) and 'dense/bias', in the slot the MTL kinds call '3C'.
        * Doukhan / Papakostas: the MTL kinds' trunks; any input whose layers all keep one output pixel (the reference's Doukhan
        * input is 21 x 68).  Jang: ONE mel-scale layer over the whole (n_fft/2 + 1, W) image -- tensors 'melCl{i}/kernel', n_mels
        * 0 = 64 -- then tanh, three times [Conv2D 3x3 'same' + BN + ReLU + Dropout(0.4) + MaxPooling2D 2x2 'valid'], Flatten, the
        * Dense; kernel_regularizer = l1_l2() (l1 = l2 = 0.01) on the mel kernels and nowhere else.
        * Training: d_y (N, n_classes) one-hot; n_classes == 2 is Keras' binary_crossentropy on the two softmax outputs with BINARY
        * accuracy, 3 categorical (the arithmetic of SMH_HEADS_SINGLE above); d_drop_heads and h_loss_weights may be NULL;
        * d_losses is four floats [loss, loss, accuracy, penalty]. */
       SMH_CNN_DOUKHAN_SINGLE = 3, SMH_CNN_PAPAKOSTAS_SINGLE = 4, SMH_CNN_JANG_SINGLE = 5 };
typedef struct smh_cnn_cfg {
    int32_t kind;      /* SMH_CNN_* */
    int32_t in_h;      /* 2*n_mels (Doukhan), 2*(n_fft/2+1) (Papakostas, Jang) */
    int32_t in_w;      /* patch width W */
    int32_t n_classes; /* 3 or 5; the *_SINGLE kinds: 2 or 3 */
    int32_t n_mels;    /* Jang: mel-scale kernels per half (0 = 120; SMH_CNN_JANG_SINGLE: 0 = 64) */
    int32_t n_fft;     /* Jang: 0 = 512 */
    int32_t fc_width;  /* Papakostas: width of the two Dense layers (0 = 4096) */
    float fs;          /* Jang: sampling rate of the mel filter bank (0 = 16000) */
} smh_cnn_cfg;
typedef struct smh_cnn smh_cnn;
int smh_cnn_create(const smh_cnn_cfg *cfg, smh_cnn **out);
void smh_cnn_destroy(smh_cnn *m);
size_t smh_cnn_num_params(const smh_cnn *m);
int smh_cnn_out_dim(const smh_cnn *m);
int smh_cnn_feat_dim(const smh_cnn *m); /* width of the feature vector the heads read */
int smh_cnn_num_tensors(const smh_cnn *m);
/* name (<= name_cap-1 chars), shape (4 ints, unused dims 1), rank and offset (in floats) of parameter tensor i */
int smh_cnn_tensor_info(const smh_cnn *m, int i, char *name, int name_cap, int *shape4, int *ndim, size_t *offset);
int smh_cnn_set_weights(smh_cnn *m, const float *h_flat, size_t n, void *stream);
int smh_cnn_get_weights(const smh_cnn *m, float *h_flat, size_t n, void *stream);
size_t smh_cnn_workspace_bytes(const smh_cnn *m, int N);
/* d_x (N, in_h, in_w) -> d_out (N, out_dim); d_feat (N, feat_dim) optional (null to skip) */
int smh_cnn_forward_f32(const smh_cnn *m, const float *d_x, int N, float *d_out, float *d_feat, void *d_work,
                        size_t work_bytes, void *stream);
/* Mixed-precision variant ("second-priority MFMA target"): the Conv2D / Dense products take bf16
 * operands (v_mfma_f32_32x32x16_bf16; activations rounded while they are staged, kernels from a transposed bf16 copy
 * rebuilt after every weight change), f32 accumulation, epilogues, pooling, LRN, mel-scale layer and heads as in f32.
 * NOT the parity path: outputs differ from smh_cnn_forward_f32 by the bf16 rounding of the operands (tests state it). */
int smh_cnn_forward_bf16(const smh_cnn *m, const float *d_x, int N, float *d_out, float *d_feat, void *d_work,
                         size_t work_bytes, void *stream);

/* ---- a13 / a14: training step of the Conv2D MTL baselines (what model.fit runs per batch for the models compiled at
 * lib/proposed_architectures.py:499-506 / :572-580 / :750-757), all three kinds.  The trainer owns its activations,
 * gradients and optimiser state (sized for max_batch >= 2: BatchNorm needs a batch).
 *   d_x (N, H, W) images; d_y (N, out_dim) targets laid out like the forward output [S | M | (N) | R | 3C one-hot]
 *   d_drop: Dropout masks (0 or 1/(1-rate)) of the trunk, one (N, dim_i) block per Dropout layer in graph order
 *           (smh_cnn_trainer_num_dropouts / _dropout_info give dim_i and rate_i), or NULL (no dropout)
 *   d_drop_heads (N, n_heads, 16) Dropout(0.4) masks of the heads or NULL; h_loss_weights: n_heads + 1 host floats or NULL
 *   d_losses: n_heads + 4 floats out = [per-head losses..., 3C loss, weighted sum (without l2), 3C accuracy, l2 penalty]
 * smh_cnn_trainer_apply_f32: g = grad * grad_scale (+ l2 term); optimizer 0 = SGD (beta1 = momentum), 1 = Adam
 * (Keras: w -= lr*sqrt(1-b2^t)/(1-b1^t) * m / (sqrt(v) + eps)); BatchNorm moving statistics <- 0.99*old + 0.01*batch;
 * the inference epilogues of smh_cnn_forward_f32 are re-folded from the new weights.                              */
typedef struct smh_cnn_trainer smh_cnn_trainer;
int smh_cnn_trainer_create(smh_cnn *m, int max_batch, smh_cnn_trainer **out);
void smh_cnn_trainer_destroy(smh_cnn_trainer *t);
float *smh_cnn_trainer_grad_ptr(smh_cnn_trainer *t);
/* floats of the data-parallel bucket that starts at smh_cnn_trainer_grad_ptr: [gradient | BatchNorm batch statistics]
 * (all-reduce all of it: the moving statistics then follow the mean over the ranks) */
size_t smh_cnn_trainer_bucket_floats(const smh_cnn_trainer *t);
/* copy the optimiser state (Adam moments / momentum, step counter) of `src` into `dst` (same model): a trainer that has
 * to grow for a larger batch keeps its state (create the larger one, copy, destroy the old one) */
int smh_cnn_trainer_copy_state(smh_cnn_trainer *dst, const smh_cnn_trainer *src, void *stream);
int smh_cnn_trainer_num_dropouts(const smh_cnn_trainer *t);
int smh_cnn_trainer_dropout_info(const smh_cnn_trainer *t, int i, size_t *dim, float *rate);
int smh_cnn_train_step_f32(smh_cnn_trainer *t, const float *d_x, const float *d_y, int N, const float *d_drop,
                           const float *d_drop_heads, const float *h_loss_weights, float *d_losses, void *stream);
int smh_cnn_trainer_apply_f32(smh_cnn_trainer *t, int optimizer, float lr, float beta1, float beta2, float eps,
                              float grad_scale, void *stream);

/* ---- a15: the random draws of a training batch, one pass each (csrc/smh_rng.hip) ------------------------------------
 * Philox4x32-10 keyed by `seed`; `offset` selects an independent stream under the same seed (pass a per-call counter):
 * equal (seed, offset, n) give equal output, on any launch geometry.
 * smh_noise_augment_f32: d_out[i] = d_x[i] + N(0, scale) -- the generator's noise augmentation,
 *   Proposed_Work_Results.py:239-242 (np.random.normal(0, scale, shape) + np.add; the scale is drawn by the caller).
 *   d_out may be d_x (in place).  Both 16-byte aligned.
 * smh_dropout_masks_f32: d_out[0 .. n_a) = (u < keep_a ? 1 / keep_a : 0), d_out[n_a .. n_a + n_b) likewise with keep_b:
 *   the SpatialDropout1D masks (N, n_blocks, 32) and the heads' Dropout(0.4) masks (N, n_heads, 16) that
 *   smh_train_step_f32 takes, in one launch.                                                                          */
int smh_noise_augment_f32(const float *d_x, float *d_out, size_t n, float scale, unsigned long long seed,
                          unsigned long long offset, void *stream);
int smh_dropout_masks_f32(float *d_out, size_t n_a, float keep_a, size_t n_b, float keep_b, unsigned long long seed,
                          unsigned long long offset, void *stream);

/* ---- a16: the fine-tuning feed of the segmentation driver: a batch of windows out of a RESIDENT featuregram, one launch
 * (csrc/smh_gather.hip; DAFx12_Speech_Music_Detection_B3_MTL_v2.py: generator :346-436 -> get_feature_patches :260-294).
 * out[n] (time-major: [t][f], image: [f][t]) = FV[f][base[n] + (first[n] + t) % period[n]], t < W, f < F, plus N(0, noise_scale)
 * drawn exactly as smh_noise_augment_f32(out, out, N*W*F, noise_scale, seed, offset) would draw it over the finished batch
 * (noise_scale == 0: a bit copy).  The periodic form is the tile-if-short rule (:262-265): a part shorter than W is repeated, so
 * a window of it wraps inside [base, base + period); with period >= first + W it is a plain window.
 * FV is (F, T) row-major on the device; h_desc is a HOST table of N x 3 int32 (base, period, first), uploaded through a staging
 * slot of the context (so a capturing stream is refused); patch_layout as for smh_extract_patches_f32: 0 = image (N, F, W),
 * 1 = time-major (N, W, F).  d_out: 16-byte aligned.  Every offset is 64-bit (F * T may exceed 2^31).
 * Checked on the host before anything is enqueued (SMH_E_INVALID, text in smh_last_error, d_out unwritten): null pointers;
 * N < 0, W < 1, F < 1; another patch_layout; noise_scale < 0; d_out misaligned; a row with base < 0, period < 1, first < 0 or
 * base + period > T.  N == 0 returns SMH_OK and launches nothing.                                                        */
int smh_gather_windows_f32(const smh_ctx *ctx, const float *d_FV, int F, long long T, const int *h_desc, int N, int W,
                           int patch_layout, float noise_scale, unsigned long long seed, unsigned long long offset,
                           float *d_out, void *stream);

/* ---- a14: one training step = what model.fit runs per batch (Proposed_Work_Results.py:298-307) for the
 * model compiled at lib/proposed_architectures.py:156-165: BCE (S, M[, N]) + MSE (R) + CCE (3C) with optional
 * loss_weights, l2(0.01) on the Dense(16) kernels, SGD(momentum, clipnorm, lr from ExponentialDecay).
 * The trainer owns activations, gradients (canonical order) and momentum; weights stay on the device.  */
typedef struct smh_trainer smh_trainer;
int smh_trainer_create(smh_model *m, int max_batch, smh_trainer **out);
void smh_trainer_destroy(smh_trainer *t);
/* device pointer to the flat gradient (smh_model_num_params floats, canonical order): all-reduce it over
 * RCCL between smh_train_step_f32 and smh_trainer_apply_sgd_f32 for data-parallel training. */
float *smh_trainer_grad_ptr(smh_trainer *t);
/* forward (training mode) + losses + backward for one batch.
 *   d_x (N, W, n_feat); d_y (N, out_dim) targets laid out like the forward output [S | M | (N) | R | 3C one-hot]
 *   d_drop_tcn  (N, n_blocks, 32) SpatialDropout1D masks (0 or 1/(1-rate)) or NULL (no dropout)
 *   d_drop_heads (N, n_heads, 16) Dropout(0.4) masks (0 or 1/0.6) or NULL
 *   h_loss_weights: n_heads + 1 host floats in output order (NULL = all 1)
 *   d_losses: 3 * n_heads + 4 floats out = [per-head losses..., 3C loss, weighted sum (without the l2 term), 3C accuracy,
 *             l2(0.01) penalty of the Dense(16) kernels = the term Keras adds to the reported total,
 *             that penalty per head (n_heads), binary accuracy (threshold 0.5) of every sigmoid head (n_heads)] */
int smh_train_step_f32(smh_trainer *t, const float *d_x, const float *d_y, int N, const float *d_drop_tcn,
                       const float *d_drop_heads, const float *h_loss_weights, float *d_losses, void *stream);
/* The intermediate-fusion model (SMH_HEADS_FUSION).  Inference: d_xH, d_xP (N, W, n_feat) time-major -> d_out (N, out_dim)
 * [S | M | (N) | R | 3C-softmax]; d_work: smh_fusion_workspace_bytes(m, N) bytes of device scratch (the two trunks' outputs).
 * Training: as smh_train_step_f32 with two inputs; d_drop_tcn is (2, N, n_blocks, 32) -- the masks of trunk H, then of trunk P
 * -- or NULL.  The trainer's data-parallel bucket is [gradient (num_params) | BN16 batch statistics of the heads (4 x 32) | the
 * fused BatchNorm's batch means (D) and population variances (D)].  Every sum of the fusion layers runs in a fixed order (no
 * atomics): deterministic mode keeps the step bit-reproducible. */
size_t smh_fusion_workspace_bytes(const smh_model *m, int N);
int smh_fusion_forward_f32(const smh_model *m, const float *d_xH, const float *d_xP, int N, float *d_out, void *d_work,
                           size_t work_bytes, void *stream);
int smh_fusion_train_step_f32(smh_trainer *t, const float *d_xH, const float *d_xP, const float *d_y, int N,
                              const float *d_drop_tcn, const float *d_drop_heads, const float *h_loss_weights, float *d_losses,
                              void *stream);
/* The fusion model without materialised input halves.  Its trunks' first layers are per half already (trunk H reads the harmonic
 * half of the H||P featuregram, trunk P the percussive half), so the per-half layer-0 partials that smh_features_l0_f32 writes are,
 * with the right kernel, each trunk's COMPLETE first layer:
 *   smh_fusion_w0_ptr            device pointer to (2 * n_feat, 32) floats: trunk H's initial-conv kernel, then trunk P's -- the d_w0 of
 *                                smh_features_l0_f32 for this model.  Owned by the model, follows every weight change (set_weights,
 *                                the trainer's apply).  Null unless SMH_HEADS_FUSION (smh_model_w0_ptr stays null for a fusion model).
 *   smh_fusion_forward_x0_f32    d_x0p (N, 2, W, 32) as smh_features_l0_f32 wrote it with that kernel -> d_out (N, out_dim), as
 *                                smh_fusion_forward_f32 on the halves of the same patches to f32 tolerance (layer 0 sums in another
 *                                order).  d_work: smh_fusion_x0_workspace_bytes(m, N) = N * 2 * W * 32 floats (the trunk taps).
 *   smh_fusion_forward_dense_f32 dense file-level inference, the fusion model's smh_model_forward_dense_f32: d_fv (2 * n_feat, Tc),
 *                                the standardised H||P featuregram (H rows, then P rows); layer 0 of both trunks once per FRAME,
 *                                every hop-`shift` patch of smh_num_patches(Tc, W, shift) a window of it.  Returns the number of
 *                                patches; d_out (nP, out_dim).  The patches pass the trunks and the tail in chunks of 2048, so
 *                                d_work = smh_fusion_dense_workspace_bytes(m, Tc, shift) = 4 * (2 * Tc * 32 + min(nP, 2048) * 2 * W * 32)
 *                                bytes however long the featuregram is.  Needs Tc >= W, shift >= 1, n_feat a multiple of 4.
 * Both trunks run as ONE grid (a second grid row selects trunk P); SMH_FUSION_TWO_LAUNCH=1 in the environment, read per call, runs
 * them as two launches instead -- bit-identical, for A/B timing.  That switch also governs smh_fusion_forward_f32.
 * Stream-ordered, no host synchronisation; d_x0p, d_fv and d_work on 16-byte boundaries; N = 0 / no patch: no launch. */
const float *smh_fusion_w0_ptr(const smh_model *m);
size_t smh_fusion_x0_workspace_bytes(const smh_model *m, int N);
int smh_fusion_forward_x0_f32(smh_model *m, const float *d_x0p, int N, void *d_work, size_t work_bytes, float *d_out, void *stream);
size_t smh_fusion_dense_workspace_bytes(const smh_model *m, int Tc, int shift);
int smh_fusion_forward_dense_f32(smh_model *m, const float *d_fv, int Tc, int shift, void *d_work, size_t work_bytes, float *d_out,
                                 void *stream);
/* Late fusion (Late_Fusion_Results.py:388-513): an ensemble of two complete single-input models of one architecture, model H on the
 * harmonic half of the H||P featuregram and model P on the percussive half, whose '3C' outputs are blended:
 *   pred[n][c] = fl(fl(a * pH[n][c]) + fl(b * pP[n][c])),  a = (float)alpha, b = (float)(1.0 - alpha)   (no FMA: numpy's
 *   alpha * pred_H + (1 - alpha) * pred_P on float32 arrays, bit for bit),   label[n] = the first maximum of pred[n] (np.argmax).
 *   smh_late_fusion_create   both models f32 TCN models (SMH_HEADS_MTL or both SMH_HEADS_CASCADED, block_variant 0) of one geometry
 *                            (n_feat, patch_size, n_classes, stacks, dilations); anything else, or the same model twice, is
 *                            SMH_E_INVALID.  The ensemble borrows the models: they must outlive it, and it follows their weights.
 *   Every forward takes alpha in [0, 1], d_work (16-byte aligned, the entry's *_workspace_bytes) and writes d_pred (N, n_classes),
 *   d_labels (N) int32 or NULL, d_heads (2, N, out_dim) or NULL: each model's own [S | M | (N) | R | 3C], bit-identical to its
 *   smh_model_forward_f32 / _x0 / _dense output.  Both models run as ONE grid (a second grid row is model P);
 *   SMH_LATE_FUSION_TWO_LAUNCH=1 in the environment, read per call, runs two launches instead -- bit-identical, for A/B timing.
 *   smh_late_fusion_forward_f32        d_xH, d_xP (N, W, n_feat) time-major
 *   smh_late_fusion_w0_ptr             device pointer to (2 * n_feat, 32) floats, model H's initial-conv kernel then model P's: the
 *                                      d_w0 of smh_features_l0_f32 for the ensemble.  Brought up to date on `stream` whenever either
 *                                      model's weights changed since the last call.
 *   smh_late_fusion_forward_x0_f32     d_x0p (N, 2, W, 32) as smh_features_l0_f32 wrote it with that kernel: half 0 is model H's
 *                                      complete first layer, half 1 model P's
 *   smh_late_fusion_forward_dense_f32  d_fv (2 * n_feat, Tc), the standardised H||P featuregram: layer 0 of both models once per
 *                                      frame, every hop-`shift` patch a window of it, in chunks of 2048 patches; returns the patch
 *                                      count nP = smh_num_patches(Tc, W, shift); outputs sized by nP.  Needs Tc >= W, shift >= 1,
 *                                      n_feat a multiple of 4.  d_work = 4 * (2 * Tc * 32 + 2 * min(nP, 2048) * out_dim) bytes, rounded up to 16.
 * Stream-ordered, no host synchronisation; N = 0: no launch.  The models' device error words are theirs: smh_model_status on each. */
typedef struct smh_late_fusion smh_late_fusion;
int smh_late_fusion_create(smh_model *mH, smh_model *mP, smh_late_fusion **out);
void smh_late_fusion_destroy(smh_late_fusion *e);
const float *smh_late_fusion_w0_ptr(smh_late_fusion *e, void *stream);
size_t smh_late_fusion_workspace_bytes(const smh_late_fusion *e, int N);
int smh_late_fusion_forward_f32(smh_late_fusion *e, const float *d_xH, const float *d_xP, int N, double alpha, void *d_work,
                                size_t work_bytes, float *d_pred, int *d_labels, float *d_heads, void *stream);
size_t smh_late_fusion_x0_workspace_bytes(const smh_late_fusion *e, int N);
int smh_late_fusion_forward_x0_f32(smh_late_fusion *e, const float *d_x0p, int N, double alpha, void *d_work, size_t work_bytes,
                                   float *d_pred, int *d_labels, float *d_heads, void *stream);
size_t smh_late_fusion_dense_workspace_bytes(const smh_late_fusion *e, int Tc, int shift);
int smh_late_fusion_forward_dense_f32(smh_late_fusion *e, const float *d_fv, int Tc, int shift, double alpha, void *d_work,
                                      size_t work_bytes, float *d_pred, int *d_labels, float *d_heads, void *stream);
/* g = grad * grad_scale (+ l2 term); per-tensor clip to `clipnorm` (<= 0: off); v = momentum*v - lr*g; w += v;
 * BN moving statistics <- 0.99*old + 0.01*batch; operand buffers re-packed on the device.              */
int smh_trainer_apply_sgd_f32(smh_trainer *t, float lr, float momentum, float clipnorm, float grad_scale, void *stream);
/* floats of the data-parallel bucket that starts at smh_trainer_grad_ptr: [gradient (num_params) | BatchNorm batch
 * statistics of the heads (4 x 32) | cascaded models only: the concatenation BatchNorm's statistics of S and M (2 x 36);
 * fusion models only: the fused BatchNorm's statistics (2 x D)];
 * all-reduce all of it so the moving statistics follow the mean over the ranks. */
size_t smh_trainer_bucket_floats(const smh_trainer *t);
/* copy momentum / Adam moments / step counters from `src` to `dst` (same model): growing a trainer keeps its state */
int smh_trainer_copy_state(smh_trainer *dst, const smh_trainer *src, void *stream);
/* zero the optimiser state (what compiling a Keras model with a new optimiser does) */
int smh_trainer_reset_state(smh_trainer *t, void *stream);
/* Deterministic weight gradients (off by default).  The backward kernels combine the workgroups' contributions with float
 * atomics, whose arrival order -- hence the last bits of a gradient -- changes from run to run.  on = 1: contributions are
 * rounded to a 2^-36 grid and summed in 64-bit integers (integer atomics: order-independent), so two runs of the same step give
 * bit-identical gradients, data-parallel replicas stay comparable run to run, and a result can be reproduced.  Costs one extra
 * pass over the gradient and 8-byte atomics (tools/bench_train.py --deterministic states the step time). */
int smh_trainer_set_deterministic(smh_trainer *t, int on, void *stream);
/* Arithmetic of the training step's matrix products (BASELINE config 5: "mixed bf16 CNN").  dtype 0 (default): exact-f32 MFMA.
 * dtype 1: the residual blocks' FORWARD and BACKWARD run on the bf16 matrix pipe with split operands -- every f32 operand as hi + lo
 * bf16, three bf16 products per f32 product, f32 accumulators; master weights, gates, losses, heads, the Dense gradients and the
 * optimiser stay f32.  The forward's outputs are within 1e-4 of the f32 forward's; the backward agrees with the f32 backward on the same
 * forward to 2e-4 (relative L2 per tensor); against the float64 oracle the gradients sit where the forward's 1e-5 puts the relu /
 * channel-maximum gates (2-3e-2 of a tensor's norm).  Patches longer than 128 frames keep the f32 backward.
 * A cascaded model (SMH_HEADS_CASCADED) accepts dtype 0 only, and so does a model the split-bf16 forward cannot run (n_feat > 256,
 * block_variant 1): dtype 1 is refused here, not at the first step. */
int smh_trainer_set_dtype(smh_trainer *t, int dtype);
/* The checks of smh_trainer_set_dtype on a model that has no trainer yet: SMH_OK, or SMH_E_INVALID + smh_last_error. */
int smh_model_check_train_dtype(const smh_model *m, int dtype);
/* General optimiser step.  optimizer 0 = SGD (beta1 = momentum; what smh_trainer_apply_sgd_f32 calls), 1 = Adam,
 * 2 = Nadam as tf.keras 2.x implements it (momentum schedule u_t = beta1 (1 - 0.5 * 0.96^(0.004 t)); the optimiser of the
 * single-head fine-tuning in DAFx12_Speech_Music_Detection_B3_MTL_v2.py:524-526).  active_mask selects the tensors that
 * belong to the (sub-)model being trained: bit 0 the TCN trunk, bit 1 the '3C' Dense, bit 2 + h head h (dense, BatchNorm
 * incl. moving statistics, output layer); tensors outside the mask are left untouched (Model(input,
 * get_layer('M').output) owns the trunk and head M only).  clipnorm <= 0: off.                                       */
#define SMH_TRAIN_TRUNK 1u
#define SMH_TRAIN_3C 2u
#define SMH_TRAIN_HEAD(h) (4u << (h))
#define SMH_TRAIN_ALL 0xFFFFFFFFu
int smh_trainer_apply_f32(smh_trainer *t, int optimizer, float lr, float beta1, float beta2, float eps, float clipnorm,
                          float grad_scale, unsigned active_mask, void *stream);

/* ---- internal: for tests, not part of the stable interface ---------------------------------------------------------------- */
/* The feature path smh_frontend_f32 (no taps) and smh_frontend_ragged_f32 take for a clip of T frames in this context, from the
 * same decision the dispatch uses: 0 the LDS-image kernel for even T, 1 the LDS-image kernel for odd T (or with SMH_FEAT_NOPAIR),
 * 2 the streaming kernels of the ragged front end (clips beyond the LDS image), 3 the two-kernel path over the whole clip
 * (launch_hp_feat + launch_std_patch: window pairs without a block-split median kernel, clips too short for the tiled medians or
 * too long for the streaming kernels' 32-bit offsets).  -1 for a null context or T < 1. */
int smh_internal_frontend_route(const smh_ctx *ctx, int T);
/* The bin-walk plan smh_ctx_create built for this context's filterbank (host values, nothing is launched):
 * out = {feat_walk_ok, feat_pend, segments of plan 0 (hp_feat_walk_kernel), segments of plan 1 (the LDS-image kernels)}.
 * feat_pend, the most filters pending at any bin, selects features_half_kernel<2, ...> (<= 2) or <4, ...>. */
int smh_internal_feat_plan(const smh_ctx *ctx, int out[4]);

#ifdef __cplusplus
}
#endif
#endif /* SMH_H */
