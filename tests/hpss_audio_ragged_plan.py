"""Python restatement of the ragged launch plan of the HPSS resynthesis (sm_hpss_mtl_amd/csrc/smh_resynth_plan.h: rag_items,
rag_spec_floats, rag_harm_floats, rag_clip_bytes, plan_rag) -- TEST INFRASTRUCTURE, like tests/stft_plans.py."""
TILE_FRAMES = 16  # kTileFrames
HARM_BLOCK = 16   # kHarmBlock
THREADS = 256


def ceil_div(a, b):
    return -(-a // b)


def num_frames(n, n_fft, hop):
    return 0 if n < n_fft else 1 + (n - n_fft) // hop


def rag_items(T):
    return ceil_div(T, TILE_FRAMES)


def rag_spec_floats(K, T):
    return ceil_div(K * T, 4) * 4


def rag_harm_floats(K, T):
    return ceil_div(T, HARM_BLOCK) * K * HARM_BLOCK


def harm_index(K, k, t):
    """element (k, t) of the blocked image, from the clip's harm offset"""
    return ((t >> 4) * K + k) * 16 + (t & 15)


def rag_clip_bytes(K, T, stft_frames, med_frames):
    items = ceil_div(T, stft_frames) + ceil_div(T, med_frames) + rag_items(T)
    return 4 * (2 * rag_spec_floats(K, T) + rag_harm_floats(K, T)) + 64 + 8 * items


def lds_bytes(n_fft, hop):
    M = n_fft // 2
    MP = M + (M >> 4) + 2
    return 8 * (M + M + 1) + 4 * n_fft + 4 * 4 * 8 * MP + 2 * 4 * ((TILE_FRAMES - 1) * hop + n_fft)


def plan_rag(n_fft, hop, n_items):
    halo = ceil_div(n_fft, hop) - 1
    refusal = ""
    if hop > n_fft:
        refusal = "hop=%d > n_fft=%d" % (hop, n_fft)
    elif halo > TILE_FRAMES:
        refusal = "more than %d overlapping frames per sample" % (TILE_FRAMES + 1)
    elif lds_bytes(n_fft, hop) > 150 * 1024:
        refusal = "bytes of LDS"
    return dict(tile=TILE_FRAMES, halo=halo, pass_frames=4, threads=THREADS, grid_x=8 * ceil_div(n_items, 8), grid_y=1,
                lds=lds_bytes(n_fft, hop), refusal=refusal)
