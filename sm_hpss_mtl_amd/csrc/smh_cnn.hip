// Conv2D MTL baselines: inference forward of
//   get_Doukhan_MTL_model     /root/reference/lib/proposed_architectures.py:425-511
//   get_Papakostas_MTL_model  /root/reference/lib/proposed_architectures.py:516-588
//   get_Jang_MTL_model        /root/reference/lib/proposed_architectures.py:650-764 (mel_scale_layer :622-646)
// with the MTL heads of :25-80, behind the C ABI of include/smh.h (smh_cnn_*); and of their single-task twins
//   get_Doukhan_model / get_Papakostas_model / get_Jang_model   lib/baseline_architectures.py:62-108, 147-175, 358-442
// (kinds SMH_CNN_*_SINGLE: the trunk, Dense(n_classes) + softmax through heads_kernel with zero heads).
//
// Design (gfx950): every Conv2D and Dense is ONE implicit-GEMM kernel on the f32 matrix cores
// (v_mfma_f32_32x32x2f32): rows = output pixels (or samples), columns = output channels, K = kh*kw*Cin.  Keras
// layouts are GEMM-ready as stored -- NHWC activations, HWIO kernels = row-major [K][Cout], Dense (in, out) =
// [K][Cout], Flatten = the NHWC image itself -- so weights are used in place, no packing pass.  The im2col gather is
// done on the fly into LDS through a per-layer table k -> (input offset, dy, dx); bias and the folded inference
// BatchNorm (y = acc*scale + shift) and the activation ride in the epilogue.  Long-K / few-row GEMMs (the Dense
// layers at small batch) are split along K into ordered partial sums (deterministic, no atomics).  Max-pooling, local
// response normalisation, Jang's mel-scale kernels (240 small strided convolutions) and the heads are small
// HBM-bound VALU kernels.
#include <climits>

#include "smh_cnn_impl.h"

extern "C" int smh_cnn_create(const smh_cnn_cfg *cfg, smh_cnn **out) {
    SMH_REQUIRE(cfg && out, "smh_cnn_create: null argument");
    if (cnn_single(cfg->kind))
        SMH_REQUIRE(cfg->n_classes == 2 || cfg->n_classes == 3, "n_classes of a single-task Conv2D baseline must be 2 or 3 (got %d)",
                    cfg->n_classes);
    else
        SMH_REQUIRE(cfg->n_classes == 3 || cfg->n_classes == 5, "n_classes must be 3 or 5 (got %d)", cfg->n_classes);
    SMH_REQUIRE(cfg->in_h >= 1 && cfg->in_w >= 1, "smh_cnn_create: bad input shape");
    SMH_REQUIRE(smh_device_count() > 0, "no HIP device visible: libsmh has no CPU path");
    smh_cnn *m = new smh_cnn();
    m->cfg = *cfg;
    std::vector<MelCl> mel;
    int rc = build_graph(m, mel);
    if (rc) {
        delete m;
        return rc;
    }
    // im2col tables, folded-epilogue offsets, largest activation
    std::vector<int2> lut;
    m->max_act = (size_t)cfg->in_h * cfg->in_w;
    for (Layer &L : m->layers) {
        m->max_act = std::max(m->max_act, (size_t)L.OH * L.OW * L.OC);
        if (L.op != kConv) continue;
        L.lut_off = lut.size();
        for (int k = 0; k < L.Kp; ++k) {
            if (k < L.K) {
                const int c = k % L.C, ij = k / L.C, j = ij % L.kw, i = ij / L.kw;
                lut.push_back(int2{(i * L.W + j) * L.C + c, (i & 0xffff) | (j << 16)});
            } else {
                lut.push_back(int2{0, 0x7fff | (0x7fff << 16)});  // out of every image: contributes zero
            }
        }
        L.es_off = m->n_fold;
        m->n_fold += 2 * (size_t)L.OC;
        L.wbf_off = m->n_wbf;
        m->n_wbf += (size_t)L.OC * L.Kp;
    }
    hipError_t e = hipMalloc((void **)&m->d_flat, m->n_params * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void **)&m->d_fold, std::max<size_t>(m->n_fold, 1) * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void **)&m->d_lut, std::max<size_t>(lut.size(), 1) * sizeof(int2));
    if (e == hipSuccess && !mel.empty()) e = hipMalloc((void **)&m->d_mel, mel.size() * sizeof(MelCl));
    if (e == hipSuccess) e = hipMemcpy(m->d_lut, lut.data(), lut.size() * sizeof(int2), hipMemcpyHostToDevice);
    if (e == hipSuccess && !mel.empty()) e = hipMemcpy(m->d_mel, mel.data(), mel.size() * sizeof(MelCl), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(m->d_flat, 0, m->n_params * sizeof(float));
    if (e != hipSuccess) {
        smh_cnn_destroy(m);
        return smh::set_error(SMH_E_HIP, "smh_cnn_create: device allocation failed: %s", hipGetErrorString(e));
    }
    m->h_flat.assign(m->n_params, 0.f);
    *out = m;
    return SMH_OK;
}

extern "C" void smh_cnn_destroy(smh_cnn *m) {
    if (!m) return;
    (void)hipFree(m->d_flat);
    (void)hipFree(m->d_fold);
    (void)hipFree(m->d_lut);
    (void)hipFree(m->d_mel);
    (void)hipFree(m->d_wbf);
    delete m;
}

extern "C" size_t smh_cnn_num_params(const smh_cnn *m) { return m ? m->n_params : 0; }
extern "C" int smh_cnn_out_dim(const smh_cnn *m) { return m ? m->out_dim : SMH_E_INVALID; }
extern "C" int smh_cnn_feat_dim(const smh_cnn *m) { return m ? m->feat_dim : SMH_E_INVALID; }
extern "C" int smh_cnn_num_tensors(const smh_cnn *m) { return m ? (int)m->tensors.size() : SMH_E_INVALID; }

extern "C" int smh_cnn_tensor_info(const smh_cnn *m, int i, char *name, int name_cap, int *shape4, int *ndim,
                                   size_t *offset) {
    SMH_REQUIRE(m, "smh_cnn_tensor_info: null model");
    SMH_REQUIRE(i >= 0 && i < (int)m->tensors.size(), "smh_cnn_tensor_info: index %d out of range", i);
    const Tensor &t = m->tensors[i];
    if (name && name_cap > 0) {
        std::strncpy(name, t.name.c_str(), (size_t)name_cap - 1);
        name[name_cap - 1] = 0;
    }
    if (shape4)
        for (int d = 0; d < 4; ++d) shape4[d] = t.shape[d];
    if (ndim) *ndim = t.ndim;
    if (offset) *offset = t.off;
    return SMH_OK;
}

extern "C" int smh_cnn_set_weights(smh_cnn *m, const float *h, size_t n, void *stream) {
    SMH_REQUIRE(m && h, "smh_cnn_set_weights: null argument");
    SMH_REQUIRE(n == m->n_params, "smh_cnn_set_weights: got %zu floats, model has %zu", n, m->n_params);
    hipStream_t st = (hipStream_t)stream;
    m->h_flat.assign(h, h + n);
    // fold bias + inference BatchNorm into y = acc * scale + shift
    std::vector<float> fold(m->n_fold);
    for (const Layer &L : m->layers) {
        if (L.op != kConv) continue;
        float *es = fold.data() + L.es_off, *eb = es + L.OC;
        const float *bias = L.t_bias >= 0 ? h + m->tensors[L.t_bias].off : nullptr;
        for (int c = 0; c < L.OC; ++c) {
            float s = 1.f, t = 0.f;
            if (L.t_bn >= 0) {
                const float *g = h + m->tensors[L.t_bn].off;
                const float gamma = g[c], beta = g[L.OC + c], mean = g[2 * L.OC + c], var = g[3 * L.OC + c];
                s = gamma / std::sqrt(var + kBnEps);
                t = beta - mean * s;
            }
            es[c] = s;
            eb[c] = (bias ? bias[c] * s : 0.f) + t;
        }
    }
    m->wbf_valid = false;
    SMH_CHECK_HIP(hipMemcpyAsync(m->d_flat, h, n * sizeof(float), hipMemcpyHostToDevice, st));
    if (m->n_fold) SMH_CHECK_HIP(hipMemcpyAsync(m->d_fold, fold.data(), m->n_fold * sizeof(float), hipMemcpyHostToDevice, st));
    SMH_CHECK_HIP(hipStreamSynchronize(st));  // host staging buffers die here
    return SMH_OK;
}

extern "C" int smh_cnn_get_weights(const smh_cnn *m, float *h, size_t n, void *stream) {
    SMH_REQUIRE(m && h, "smh_cnn_get_weights: null argument");
    SMH_REQUIRE(n == m->n_params, "smh_cnn_get_weights: got room for %zu floats, model has %zu", n, m->n_params);
    // the device copy is the master: a trainer (smh_cnn_train.hip) updates it in place
    hipStream_t st = (hipStream_t)stream;
    SMH_CHECK_HIP(hipMemcpyAsync(h, m->d_flat, n * sizeof(float), hipMemcpyDeviceToHost, st));
    SMH_CHECK_HIP(hipStreamSynchronize(st));
    return SMH_OK;
}

extern "C" size_t smh_cnn_workspace_bytes(const smh_cnn *m, int N) {
    if (!m || N < 0) return 0;
    return carve(m, nullptr, N).bytes;
}

static int forward_impl(const smh_cnn *m, const float *d_x, int N, float *d_out, float *d_feat, void *d_work,
                        size_t work_bytes, void *stream, bool bf16);

extern "C" int smh_cnn_forward_f32(const smh_cnn *m, const float *d_x, int N, float *d_out, float *d_feat, void *d_work,
                                   size_t work_bytes, void *stream) {
    return forward_impl(m, d_x, N, d_out, d_feat, d_work, work_bytes, stream, false);
}

extern "C" int smh_cnn_forward_bf16(const smh_cnn *m, const float *d_x, int N, float *d_out, float *d_feat, void *d_work,
                                    size_t work_bytes, void *stream) {
    return forward_impl(m, d_x, N, d_out, d_feat, d_work, work_bytes, stream, true);
}

static int forward_impl(const smh_cnn *m, const float *d_x, int N, float *d_out, float *d_feat, void *d_work,
                        size_t work_bytes, void *stream, bool bf16) {
    SMH_REQUIRE(m, "smh_cnn_forward_f32: null model");
    SMH_REQUIRE(N >= 0, "smh_cnn_forward_f32: negative batch");
    if (N == 0) return SMH_OK;
    SMH_REQUIRE(d_x && d_out && d_work, "smh_cnn_forward_f32: null argument");
    const Work w = carve(m, d_work, N);
    if (work_bytes < w.bytes)
        return smh::set_error(SMH_E_WORKSPACE, "smh_cnn_forward_f32: workspace too small (%zu < %zu bytes)", work_bytes, w.bytes);
    hipStream_t st = (hipStream_t)stream;
    if (bf16 && !m->wbf_valid) {  // bf16 operand cache: every kernel transposed to [Cout][Kp], once per weight version
        if (!m->d_wbf) SMH_CHECK_HIP(hipMalloc(&m->d_wbf, std::max<size_t>(m->n_wbf, 1) * sizeof(__bf16)));
        for (const Layer &L : m->layers)
            if (L.op == kConv) {
                const size_t tot = (size_t)L.OC * L.Kp;
                hipLaunchKernelGGL(pack_wt_bf16_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st,
                                   (const float *)(m->d_flat + m->tensors[L.t_kernel].off), L.K, L.Kp, L.OC,
                                   reinterpret_cast<__bf16 *>(m->d_wbf) + L.wbf_off);
            }
        int rcp = smh::launch_status("pack_wt_bf16_kernel");
        if (rcp) return rcp;
        m->wbf_valid = true;
    }
    const size_t in_floats = (size_t)m->cfg.in_h * m->cfg.in_w;
    for (int n0 = 0; n0 < N; n0 += kChunk) {
        const int n = std::min(kChunk, N - n0);
        const float *src = d_x + (size_t)n0 * in_floats;
        int pp = 0;
        for (const Layer &L : m->layers) {
            float *dst = w.act[pp];
            if (L.op == kConv) {
                SMH_REQUIRE(L.OC % 4 == 0, "smh_cnn: Cout=%d is not a multiple of 4", L.OC);
                ConvArgs a = conv_args(m, L, n);
                a.x = src, a.w = m->d_flat + m->tensors[L.t_kernel].off;
                a.es = m->d_fold + L.es_off, a.eb = a.es + L.OC, a.act = L.act;
                a.y = dst, a.partial = w.partial;
                const GemmPlan p = plan_forward(m->cfg.kind, L, n, bf16);
                if (bf16) {  // the same plan on the bf16 kernel's k-steps, the transposed bf16 kernels as a second operand
                    a.ksplit = p.ksplit, a.ksteps = p.ksteps, a.ksteps_per = p.ksteps_per;
                    const dim3 grid(p.mt, p.nt, p.ksplit);
                    const __bf16 *wt = reinterpret_cast<const __bf16 *>(m->d_wbf) + L.wbf_off;
                    if (p.bn == 64) hipLaunchKernelGGL(conv_gemm_bf16_kernel<64>, grid, dim3(256), 0, st, a, wt);
                    else hipLaunchKernelGGL(conv_gemm_bf16_kernel<128>, grid, dim3(256), 0, st, a, wt);
                    finish_split<0>(a, p, st);
                } else {
                    launch_conv_gemm<0>(a, p, st);
                }
            } else if (L.op == kPool) {
                const size_t total = (size_t)n * L.OH * L.OW * L.C;
                hipLaunchKernelGGL(maxpool_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, src, L.H, L.W,
                                   L.C, L.OH, L.OW, L.kh, L.kw, L.sh, L.sw, L.pt, L.pl, total, dst);
            } else if (L.op == kLrnRelu) {
                const size_t total = (size_t)n * L.H * L.W * L.C;
                hipLaunchKernelGGL(lrn_relu_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, src, L.C, 5,
                                   1e-4f, 0.75f, total, dst);
            } else {  // kMelCl
                const size_t total = (size_t)n * L.OH * L.OW;
                hipLaunchKernelGGL(melcl_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, src,
                                   (const MelCl *)m->d_mel, (const float *)m->d_flat, L.H, L.W, L.OH, L.kw, total, dst);
            }
            src = dst;
            pp ^= 1;
        }
        // src now holds the (n, feat_dim) features
        if (d_feat)
            SMH_CHECK_HIP(hipMemcpyAsync(d_feat + (size_t)n0 * m->feat_dim, src, (size_t)n * m->feat_dim * sizeof(float),
                                         hipMemcpyDeviceToDevice, st));
        HeadArgs ha{};
        const float *F = m->d_flat;
        ha.c3k = F + m->tensors[m->t_c3].off, ha.c3b = F + m->tensors[m->t_c3 + 1].off;
        for (int h = 0; h < m->n_heads; ++h) {
            const int t = m->t_head[h];
            ha.hk[h] = F + m->tensors[t].off, ha.hb[h] = F + m->tensors[t + 1].off;
            ha.hbn[h] = F + m->tensors[t + 2].off;  // gamma, beta, mean, var are contiguous
            ha.ok[h] = F + m->tensors[t + 6].off, ha.ob[h] = F + m->tensors[t + 7].off;
            ha.odim[h] = m->odim[h], ha.sigm[h] = m->sigm[h];
        }
        ha.D = m->feat_dim, ha.n_classes = m->cfg.n_classes, ha.n_heads = m->n_heads, ha.out_dim = m->out_dim;
        hipLaunchKernelGGL(heads_kernel, dim3(n), dim3(256), 0, st, src, ha, d_out + (size_t)n0 * m->out_dim);
    }
    return smh::launch_status("smh_cnn forward");
}

// tests: the launch plan of layer `layer` under the current switches, from the functions the launchers call.  what = 0 / 1: inference
// forward of one pass of N images, f32 / bf16; 2: training forward; 3: weight gradient; 4: data gradient (2-4: a batch of N, a partial
// buffer of cap_floats); 5: a column reduction over the layer's (N * OH * OW) x OC output.  out = {bn, mt, nt, ksteps, ksplit,
// ksteps_per, partial_floats, 0}; a small-K weight gradient {0, 0, 0, 0, nb, rows_per_block, partial_floats, 1}; a column reduction
// {vec, slabs, rows_per_pass, rows_per_block, blocks, 0, 0, 0}.  Returns 0, or -1 where the layer has no such launch -- or where a
// count does not fit an int (no graph comes near: a split GEMM has fewer than 256 tiles, so at most 16 * 256 * 128 * 128 = 67 M floats
// of forward partials, and the other partials are bounded by cap_floats).
extern "C" int smh_internal_cnn_plan(const smh_cnn *m, int layer, int what, int N, size_t cap_floats, int out[8]) {
    if (!m || layer < 0 || layer >= (int)m->layers.size() || N < 1 || m->layers[layer].op != kConv) return -1;
    const Layer &L = m->layers[layer];
    const CnnSwitches sw = read_cnn_switches();
    GemmPlan g{};
    int v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (what == 0 || what == 1) {
        g = plan_forward(m->cfg.kind, L, N, what == 1);
    } else if (what == 2) {
        g = plan_train_forward(L, N, cap_floats);
    } else if (what == 3) {
        const WgradPlan w = plan_wgrad(L, N, cap_floats, sw);
        g = w.gemm;
        g.partial_floats = w.partial_floats;
        if (w.smallk) v[4] = w.nb, v[5] = w.rows_per_block, v[7] = 1;
    } else if (what == 4 && layer > 0) {
        g = plan_dgrad(L, N, cap_floats, sw);
    } else if (what == 5) {
        const ColReducePlan c = plan_col_reduce((size_t)N * L.OH * L.OW, L.OC);
        if (c.rows_per_block > INT_MAX || c.blocks > INT_MAX) return -1;
        const int cv[8] = {c.vec, (int)c.slabs, (int)c.rows_per_pass, (int)c.rows_per_block, (int)c.blocks, 0, 0, 0};
        std::copy(cv, cv + 8, out);
        return 0;
    } else {
        return -1;
    }
    if (g.partial_floats > INT_MAX) return -1;
    if (!v[7]) v[0] = g.bn, v[1] = g.mt, v[2] = g.nt, v[3] = g.ksteps, v[4] = g.ksplit, v[5] = g.ksteps_per;
    v[6] = (int)g.partial_floats;
    std::copy(v, v + 8, out);
    return 0;
}

// tests: floats of the partial buffer a trainer of this model for max_batch images allocates
extern "C" size_t smh_internal_cnn_partial_floats(const smh_cnn *m, int max_batch) {
    return m ? trainer_partial_floats(m->layers, max_batch) : 0;
}
