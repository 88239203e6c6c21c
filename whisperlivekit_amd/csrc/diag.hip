// Kernel-level diagnostics behind the C ABI: run ONE kernel on host data and hand the result back,
// so the GPU parity tests can compare each building block with a plain fp32 reference.
#include <cstdio>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/wlk_hip.h"
#include "common.h"
#include "decoder_chain.h"
#include "internal.h"
#include "nllb_internal.h"
#include "wave_ops.h"

using namespace wlk;

namespace {
thread_local std::string g_diag_error;
struct DevBuf {
    float* p = nullptr;
    explicit DevBuf(size_t n, const float* host = nullptr) {
        WLK_HIP(hipMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(n, 1) * sizeof(float)));
        if (host) WLK_HIP(hipMemcpy(p, host, n * sizeof(float), hipMemcpyHostToDevice));
    }
    ~DevBuf() { (void)hipFree(p); }
};
template <typename F>
int run(F&& f) {
    try {
        f();
        WLK_HIP(hipDeviceSynchronize());
        return WLK_OK;
    } catch (const std::exception& e) {
        g_diag_error = e.what();
        return WLK_ERR_HIP;
    }
}
}  // namespace

void wlk::set_diag_error(const std::string& msg) { g_diag_error = msg; }

// wave_ops.h against the __shfl_xor loops it replaces: out[0..9][lane] = VALU-butterfly results, ref[0..9][lane] = the
// shuffle forms, on the same 64 floats (rows: sum, max, row16 sum 1-2-4-8, xor 1, 2, 4, 8, 16, 32, arg-max index)
__global__ __launch_bounds__(64) void wave_ops_probe_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                            float* __restrict__ ref) {
    const int lane = threadIdx.x;
    const float v = in[lane];
    out[0 * 64 + lane] = wave_sum(v);
    out[1 * 64 + lane] = wave_max(v);
    out[2 * 64 + lane] = row16_sum_1248(v);
    out[3 * 64 + lane] = wave_xor<1>(v);
    out[4 * 64 + lane] = wave_xor<2>(v);
    out[5 * 64 + lane] = wave_xor<4>(v);
    out[6 * 64 + lane] = wave_xor<8>(v);
    out[7 * 64 + lane] = wave_xor<16>(v);
    out[8 * 64 + lane] = wave_xor<32>(v);
    {
        float bv = v;
        int bi = lane;
        wave_argmax(bv, bi);
        out[9 * 64 + lane] = (float)bi;
    }
    float s = v, m = v, r = v;
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
    for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    r += __shfl_xor(r, 1, 64);
    r += __shfl_xor(r, 2, 64);
    r += __shfl_xor(r, 4, 64);
    r += __shfl_xor(r, 8, 64);
    ref[0 * 64 + lane] = s;
    ref[1 * 64 + lane] = m;
    ref[2 * 64 + lane] = r;
    ref[3 * 64 + lane] = __shfl_xor(v, 1, 64);
    ref[4 * 64 + lane] = __shfl_xor(v, 2, 64);
    ref[5 * 64 + lane] = __shfl_xor(v, 4, 64);
    ref[6 * 64 + lane] = __shfl_xor(v, 8, 64);
    ref[7 * 64 + lane] = __shfl_xor(v, 16, 64);
    ref[8 * 64 + lane] = __shfl_xor(v, 32, 64);
    {
        float bv = v;
        int bi = lane;
        for (int off = 32; off >= 1; off >>= 1) {
            const float ov = __shfl_xor(bv, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        ref[9 * 64 + lane] = (float)bi;
    }
}

extern "C" {

const char* wlk_diag_last_error(void) { return g_diag_error.c_str(); }

int wlk_diag_linear(const float* a, int64_t lda, int64_t a_floats, const float* w, const float* bias, const float* r,
                    int64_t ldr, int m, int n, int k, int flags, float scale, int scale_cols, int force_gemv, float* c) {
    return run([&]() {
        DevBuf A(a_floats, a), W((size_t)n * k, w), B(n, bias), R(r ? (size_t)m * ldr : 1, r), Cc((size_t)m * n);
        GemmArgs g;
        g.A = A.p; g.lda = lda; g.W = W.p; g.bias = bias ? B.p : nullptr; g.C = Cc.p; g.ldc = n;
        g.R = r ? R.p : nullptr; g.ldr = ldr; g.M = m; g.N = n; g.K = k; g.flags = flags; g.scale = scale;
        g.scale_cols = scale_cols;
        LaunchCtx ctx;
        g.force_kwave = force_gemv == 2;
        g.force_kernel = (force_gemv >= 2 && force_gemv <= 4) || (force_gemv >= 6 && force_gemv <= 8) ? force_gemv : 0;
        if (force_gemv == 1) launch_gemv(ctx, g, "diag_gemv");
        else if (force_gemv >= 5 && force_gemv <= 8) launch_gemm_kp(ctx, g, "diag_gemm_kp");      // 6 / 7: 16 x 16 / 32 x 32 tiles below 512 rows
        else launch_gemm(ctx, g, "diag_gemm");
        WLK_HIP(hipDeviceSynchronize());
        WLK_HIP(hipMemcpy(c, Cc.p, (size_t)m * n * sizeof(float), hipMemcpyDeviceToHost));
    });
}

/* average microseconds per launch of `reps` back-to-back launches of one linear layer (device-resident operands,
 * HIP events around the whole train, one warm-up launch first): the kernel-tuning probe */
int wlk_diag_linear_time(int m, int n, int k, int flags, int force, int reps, float* us_per_launch) {
    return run([&]() {
        std::vector<float> ha((size_t)m * k), hw((size_t)n * k);
        unsigned seed = 12345u;
        auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return ((seed >> 8) & 0xffff) / 65536.0f - 0.5f; };
        for (auto& v : ha) v = rnd();
        for (auto& v : hw) v = rnd() * 0.05f;
        DevBuf A((size_t)m * k, ha.data()), W((size_t)n * k, hw.data()), B(n), R((size_t)m * n), Cc((size_t)m * n);
        WLK_HIP(hipMemset(B.p, 0, n * sizeof(float)));
        WLK_HIP(hipMemset(R.p, 0, (size_t)m * n * sizeof(float)));
        GemmArgs g;
        g.A = A.p; g.lda = k; g.W = W.p; g.bias = B.p; g.C = Cc.p; g.ldc = n; g.R = (flags & kGemmResidual) ? R.p : nullptr;
        g.ldr = n; g.M = m; g.N = n; g.K = k; g.flags = flags; g.scale = 0.5f; g.scale_cols = n / 2;
        g.force_kwave = force == 2;
        g.force_kernel = (force >= 2 && force <= 4) || (force >= 6 && force <= 8) || force >= 500 ? force : 0;      // >= 500: kp family with the tile (force - 500) / 10 x % 10
        long long* dbg = nullptr;
        const bool want_clock = getenv("WLK_GEMM_CLOCKS") != nullptr;
        if (want_clock) {
            WLK_HIP(hipMalloc(reinterpret_cast<void**>(&dbg), 4 * 8192 * sizeof(long long)));
            WLK_HIP(hipMemset(dbg, 0, 4 * 8192 * sizeof(long long)));
            g.dbg_clock = dbg;
        }
        hipStream_t st;
        WLK_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        LaunchCtx ctx{st, nullptr};
        auto go = [&]() {
            if (force == 1) launch_gemv(ctx, g, "diag");
            else if ((force >= 5 && force <= 8) || force >= 500) launch_gemm_kp(ctx, g, "diag");
            else launch_gemm(ctx, g, "diag");
        };
        go();
        WLK_HIP(hipStreamSynchronize(st));
        hipEvent_t e0, e1;
        WLK_HIP(hipEventCreate(&e0));
        WLK_HIP(hipEventCreate(&e1));
        WLK_HIP(hipEventRecord(e0, st));
        for (int i = 0; i < reps; ++i) go();
        WLK_HIP(hipEventRecord(e1, st));
        WLK_HIP(hipStreamSynchronize(st));
        float ms = 0.f;
        WLK_HIP(hipEventElapsedTime(&ms, e0, e1));
        *us_per_launch = 1e3f * ms / (float)reps;
        if (want_clock) {
            std::vector<long long> h(4 * 8192);
            WLK_HIP(hipMemcpy(h.data(), dbg, h.size() * sizeof(long long), hipMemcpyDeviceToHost));
            long long t0 = 0, t1 = 0;
            double pro = 0, loop = 0, epi = 0;
            int n = 0;
            for (int i = 0; i < 8192; ++i) {
                if (!h[4 * i + 3]) continue;
                if (!n || h[4 * i] < t0) t0 = h[4 * i];
                if (!n || h[4 * i + 3] > t1) t1 = h[4 * i + 3];
                pro += h[4 * i + 1] - h[4 * i]; loop += h[4 * i + 2] - h[4 * i + 1]; epi += h[4 * i + 3] - h[4 * i + 2];
                ++n;
            }
            if (n) fprintf(stderr, "[clocks] %d workgroups: prologue %.0f, loop %.0f, fold+epilogue %.0f ticks (mean); first start -> last end %lld ticks\n",
                           n, pro / n, loop / n, epi / n, t1 - t0);
            (void)hipFree(dbg);
        }
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        (void)hipStreamDestroy(st);
    });
}

int wlk_diag_linear_ln(const float* a, const float* w, const float* bias, const float* gamma, const float* beta, int m,
                       int n, int k, int force_gemv, float* c) {
    return run([&]() {
        DevBuf A((size_t)m * k, a), W((size_t)n * k, w), B(n, bias), G(k, gamma), Bt(k, beta), Cc((size_t)m * n);
        GemmArgs g;
        g.A = A.p; g.lda = k; g.W = W.p; g.bias = B.p; g.C = Cc.p; g.ldc = n; g.M = m; g.N = n; g.K = k;
        g.ln_gamma = G.p; g.ln_beta = Bt.p;
        LaunchCtx ctx;
        (void)force_gemv;
        if (m <= 8) launch_gemv(ctx, g, "diag_gemv_ln");     // decode steps: the weight-streaming kernels
        else launch_gemm(ctx, g, "diag_gemm_ln");            // more rows: throws (no MFMA kernel takes the LayerNorm)
        WLK_HIP(hipDeviceSynchronize());
        WLK_HIP(hipMemcpy(c, Cc.p, (size_t)m * n * sizeof(float), hipMemcpyDeviceToHost));
    });
}

int wlk_diag_layernorm(const float* x, const float* gamma, const float* beta, int rows, int d, float* y) {
    return run([&]() {
        DevBuf X((size_t)rows * d, x), G(d, gamma), Bt(d, beta), Y((size_t)rows * d);
        LaunchCtx ctx;
        launch_layernorm(ctx, X.p, d, G.p, Bt.p, Y.p, d, rows, d, "diag_ln");
        WLK_HIP(hipDeviceSynchronize());
        WLK_HIP(hipMemcpy(y, Y.p, (size_t)rows * d * sizeof(float), hipMemcpyDeviceToHost));
    });
}

int wlk_diag_prefill_stack(wlk_session** sessions, const int64_t* tokens, const int32_t* n_tok, const int32_t* sot_index, int32_t n,
                           int32_t* taken) {
    if (!sessions || !tokens || !n_tok || !sot_index || !taken || n < 1 || n > kMaxBatch) {
        set_last_error("prefill_stack: bad arguments");
        return WLK_ERR_ARG;
    }
    return run([&]() {
        wlk_model* m = sessions[0]->m;
        WLK_HIP(hipSetDevice(m->device));
        wlk_prefill_ws ws;
        wlk_prefill_ws_alloc(m, ws, kMaxBatch, std::min(256, (int)m->D.n_text_ctx));
        hipStream_t st = nullptr;
        try {
            WLK_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
            std::vector<wlk_prefill_item> items(n);
            std::vector<wlk_prefill_item*> stack;
            const int64_t* t = tokens;
            for (int i = 0; i < n; ++i) {
                items[i].s = sessions[i];
                items[i].tokens = t;
                items[i].n_tok = n_tok[i];
                items[i].sot_index = sot_index[i];
                t += n_tok[i];
                WLK_HIP(hipStreamSynchronize(sessions[i]->stream));
                taken[i] = sessions[i]->m == m && wlk_prefill_precheck(items[i], ws).empty() ? 1 : 0;
                if (taken[i]) stack.push_back(&items[i]);
            }
            wlk_prefill_group(stack, LaunchCtx{st, nullptr}, ws);
            WLK_HIP(hipStreamSynchronize(st));
        } catch (...) {
            if (st) (void)hipStreamDestroy(st);
            wlk_prefill_ws_free(ws);
            throw;
        }
        (void)hipStreamDestroy(st);
        wlk_prefill_ws_free(ws);
    });
}

int wlk_diag_encoder_attention_time(int t, int d, int n_head, int reps, float* us_per_launch) {
    return run([&]() {
        std::vector<float> h((size_t)t * 3 * d);
        unsigned seed = 777u;
        for (auto& v : h) { seed = seed * 1664525u + 1013904223u; v = (((seed >> 8) & 0xffff) / 65536.0f - 0.5f) * 1.5f; }
        DevBuf Q((size_t)t * 3 * d, h.data()), O((size_t)t * d);

        hipStream_t st;
        WLK_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        LaunchCtx ctx{st, nullptr};
        auto go = [&]() { launch_encoder_attention(ctx, Q.p, O.p, t, d, n_head); };
        go();
        WLK_HIP(hipStreamSynchronize(st));
        hipEvent_t e0, e1;
        WLK_HIP(hipEventCreate(&e0));
        WLK_HIP(hipEventCreate(&e1));
        WLK_HIP(hipEventRecord(e0, st));
        for (int i = 0; i < reps; ++i) go();
        WLK_HIP(hipEventRecord(e1, st));
        WLK_HIP(hipStreamSynchronize(st));
        float ms = 0.f;
        WLK_HIP(hipEventElapsedTime(&ms, e0, e1));
        *us_per_launch = 1e3f * ms / (float)reps;
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        (void)hipStreamDestroy(st);
    });
}

int wlk_diag_encoder_attention(const float* qkv, int t, int d, int n_head, float* out) {
    return run([&]() {
        DevBuf Q((size_t)t * 3 * d, qkv), O((size_t)t * d);
        LaunchCtx ctx;
        launch_encoder_attention(ctx, Q.p, O.p, t, d, n_head);
        WLK_HIP(hipDeviceSynchronize());
        WLK_HIP(hipMemcpy(out, O.p, (size_t)t * d * sizeof(float), hipMemcpyDeviceToHost));
    });
}

int wlk_diag_env_refresh(void) {
    wlk::refresh_env_switches();
    return 0;
}

int wlk_diag_wave_ops(const float* in64, float* out640, float* ref640) {
    return run([&]() {
        DevBuf I(64, in64), O(640), R(640);
        hipLaunchKernelGGL(wave_ops_probe_kernel, dim3(1), dim3(64), 0, nullptr, I.p, O.p, R.p);
        WLK_HIP(hipGetLastError());
        WLK_HIP(hipDeviceSynchronize());
        WLK_HIP(hipMemcpy(out640, O.p, 640 * sizeof(float), hipMemcpyDeviceToHost));
        WLK_HIP(hipMemcpy(ref640, R.p, 640 * sizeof(float), hipMemcpyDeviceToHost));
    });
}

/* C[m, n] = epilogue(A[m, k] . W[n, k]^T + bias) through the X3 path (gemm_x3.hip): both operands are packed into three
 * bf16 planes on the device, the wide bf16-MFMA kernel runs, the fp32 result comes back */
int wlk_diag_linear_x3(const float* a, const float* w, const float* bias, int m, int n, int k, int flags, float scale,
                       int scale_cols, float* c) {
    return run([&]() {
        DevBuf A((size_t)m * k, a), W((size_t)n * k, w), B(n, bias), Cc((size_t)m * n);
        unsigned short *a3 = nullptr, *w3 = nullptr;
        WLK_HIP(hipMalloc(reinterpret_cast<void**>(&a3), (size_t)m * 3 * k * sizeof(unsigned short)));
        WLK_HIP(hipMalloc(reinterpret_cast<void**>(&w3), x3_w_elems(n, k) * sizeof(unsigned short)));
        LaunchCtx ctx;
        launch_x3_pack(ctx, A.p, k, a3, k, m, k);
        launch_x3_pack_w(ctx, W.p, k, w3, n, k);
        X3GemmArgs g;
        g.A3 = a3; g.lda = k; g.W3 = w3; g.bias = bias ? B.p : nullptr; g.C = Cc.p; g.ldc = n; g.M = m; g.N = n; g.K = k;
        g.flags = flags; g.scale = scale; g.scale_cols = scale_cols;
        launch_gemm_x3(ctx, g, "diag_x3");
        WLK_HIP(hipDeviceSynchronize());
        WLK_HIP(hipMemcpy(c, Cc.p, (size_t)m * n * sizeof(float), hipMemcpyDeviceToHost));
        (void)hipFree(a3);
        (void)hipFree(w3);
    });
}

/* kernel-tuning probe: average microseconds per launch of the X3 wide GEMM (device-resident pseudo-random operands) */
int wlk_diag_linear_x3_time(int m, int n, int k, int flags, int reps, float* us_per_launch) {
    return run([&]() {
        std::vector<float> ha((size_t)m * k), hw((size_t)n * k);
        unsigned seed = 12345u;
        auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return ((seed >> 8) & 0xffff) / 65536.0f - 0.5f; };
        for (auto& v : ha) v = rnd();
        for (auto& v : hw) v = rnd() * 0.05f;
        DevBuf A((size_t)m * k, ha.data()), W((size_t)n * k, hw.data()), B(n), Cc((size_t)m * n);
        WLK_HIP(hipMemset(B.p, 0, n * sizeof(float)));
        unsigned short *a3 = nullptr, *w3 = nullptr;
        WLK_HIP(hipMalloc(reinterpret_cast<void**>(&a3), (size_t)m * 3 * k * sizeof(unsigned short)));
        WLK_HIP(hipMalloc(reinterpret_cast<void**>(&w3), x3_w_elems(n, k) * sizeof(unsigned short)));
        hipStream_t st;
        WLK_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        LaunchCtx ctx{st, nullptr};
        launch_x3_pack(ctx, A.p, k, a3, k, m, k);
        launch_x3_pack_w(ctx, W.p, k, w3, n, k);
        X3GemmArgs g;
        g.A3 = a3; g.lda = k; g.W3 = w3; g.bias = B.p; g.C = Cc.p; g.ldc = n; g.M = m; g.N = n; g.K = k; g.flags = flags;
        g.scale = 0.5f; g.scale_cols = n / 2;
        launch_gemm_x3(ctx, g, "diag");
        WLK_HIP(hipStreamSynchronize(st));
        hipEvent_t e0, e1;
        WLK_HIP(hipEventCreate(&e0));
        WLK_HIP(hipEventCreate(&e1));
        WLK_HIP(hipEventRecord(e0, st));
        for (int i = 0; i < reps; ++i) launch_gemm_x3(ctx, g, "diag");
        WLK_HIP(hipEventRecord(e1, st));
        WLK_HIP(hipStreamSynchronize(st));
        float ms = 0.f;
        WLK_HIP(hipEventElapsedTime(&ms, e0, e1));
        *us_per_launch = 1e3f * ms / (float)reps;
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        (void)hipStreamDestroy(st);
        (void)hipFree(a3);
        (void)hipFree(w3);
    });
}

/* LayerNorm with the result in the X3 format, unpacked again: y must equal wlk_diag_layernorm's y bit for bit */
int wlk_diag_layernorm_x3(const float* x, const float* gamma, const float* beta, int rows, int d, float* y) {
    return run([&]() {
        DevBuf X((size_t)rows * d, x), G(d, gamma), Bt(d, beta), Y((size_t)rows * d);
        unsigned short* y3 = nullptr;
        WLK_HIP(hipMalloc(reinterpret_cast<void**>(&y3), (size_t)rows * 3 * d * sizeof(unsigned short)));
        LaunchCtx ctx;
        launch_layernorm_x3(ctx, X.p, d, G.p, Bt.p, y3, d, rows, d, "diag_ln_x3");
        launch_x3_unpack(ctx, y3, d, Y.p, d, rows, d);
        WLK_HIP(hipDeviceSynchronize());
        WLK_HIP(hipMemcpy(y, Y.p, (size_t)rows * d * sizeof(float), hipMemcpyDeviceToHost));
        (void)hipFree(y3);
    });
}

/* encoder self-attention through the X3 path (attention_x3.hip): qkv [t, 3d] (q and k pre-scaled) is packed into the
 * operand image on the device, out [t, d] comes back; compare with wlk_diag_encoder_attention */
int wlk_diag_encoder_attention_x3(const float* qkv, int t, int d, int n_head, float* out) {
    return run([&]() {
        DevBuf Q((size_t)t * 3 * d, qkv), O((size_t)t * d);
        unsigned short* img = nullptr;
        const size_t n = x3_attn_image_elems(t, d);
        WLK_HIP(hipMalloc(reinterpret_cast<void**>(&img), n * sizeof(unsigned short)));
        LaunchCtx ctx;
        launch_x3_pack_qkv(ctx, Q.p, img, t, d, x3_attn_vt_off(t, d), x3_attn_vt_ld(t));
        launch_encoder_attention_x3(ctx, img, 2L * d, x3_attn_vt_off(t, d), x3_attn_vt_ld(t), O.p, d, t, d, n_head, nullptr, 0);
        WLK_HIP(hipDeviceSynchronize());
        WLK_HIP(hipMemcpy(out, O.p, (size_t)t * d * sizeof(float), hipMemcpyDeviceToHost));
        (void)hipFree(img);
    });
}

/* The PRODUCTION operand route of the X3 attention against the diagnostic one: x [t][d] . w [3 d][d]^T (+ bias, q | k columns
 * scaled) through gemm_x3 with the X3 epilogue (q | k as X3 rows, V transposed in the lane order of the attention kernel) ->
 * enc_attention_x3 -> out_epilogue; the same projection with an fp32 result -> x3_pack_qkv -> attention -> out_packed.
 * The two must agree bit for bit (same fp32 values split into the same planes, the same image). */
int wlk_diag_qkv_x3_attention(const float* x, const float* w, const float* bias, int t, int d, int n_head, float scale,
                              float* out_epilogue, float* out_packed) {
    return run([&]() {
        DevBuf X((size_t)t * d, x), W((size_t)3 * d * d, w), B((size_t)3 * d, bias), QKV((size_t)t * 3 * d), O((size_t)t * d);
        unsigned short *x3 = nullptr, *w3 = nullptr, *img = nullptr;
        const size_t n_img = x3_attn_image_elems(t, d);
        WLK_HIP(hipMalloc(reinterpret_cast<void**>(&x3), (size_t)t * 3 * d * sizeof(unsigned short)));
        WLK_HIP(hipMalloc(reinterpret_cast<void**>(&w3), x3_w_elems(3 * d, d) * sizeof(unsigned short)));
        WLK_HIP(hipMalloc(reinterpret_cast<void**>(&img), n_img * sizeof(unsigned short)));
        LaunchCtx ctx;
        launch_x3_pack(ctx, X.p, d, x3, d, t, d);
        launch_x3_pack_w(ctx, W.p, d, w3, 3 * d, d);
        X3GemmArgs g;
        g.A3 = x3; g.lda = d; g.W3 = w3; g.bias = B.p; g.M = t; g.N = 3 * d; g.K = d;
        g.flags = kGemmScaleCols; g.scale = scale; g.scale_cols = 2 * d;
        for (int route = 0; route < 2; ++route) {
            WLK_HIP(hipMemset(img, 0, n_img * sizeof(unsigned short)));     // the session's image starts zeroed as well
            X3GemmArgs r = g;
            if (route == 0) {
                r.x3_out = true; r.C3 = img; r.ldc3 = 2 * d; r.vt_col0 = 2 * d; r.vt_off = x3_attn_vt_off(t, d); r.vt_ld = x3_attn_vt_ld(t);
                launch_gemm_x3(ctx, r, "diag_qkv_x3");
            } else {
                r.C = QKV.p; r.ldc = 3 * d;
                launch_gemm_x3(ctx, r, "diag_qkv");
                launch_x3_pack_qkv(ctx, QKV.p, img, t, d, x3_attn_vt_off(t, d), x3_attn_vt_ld(t));
            }
            launch_encoder_attention_x3(ctx, img, 2L * d, x3_attn_vt_off(t, d), x3_attn_vt_ld(t), O.p, d, t, d, n_head, nullptr, 0);
            WLK_HIP(hipDeviceSynchronize());
            WLK_HIP(hipMemcpy(route == 0 ? out_epilogue : out_packed, O.p, (size_t)t * d * sizeof(float), hipMemcpyDeviceToHost));
        }
        (void)hipFree(x3);
        (void)hipFree(w3);
        (void)hipFree(img);
    });
}

/* timing probe of the same: average microseconds per launch */
int wlk_diag_encoder_attention_x3_time(int t, int d, int n_head, int reps, float* us_per_launch) {
    return run([&]() {
        std::vector<float> h((size_t)t * 3 * d);
        unsigned seed = 777u;
        for (auto& v : h) { seed = seed * 1664525u + 1013904223u; v = (((seed >> 8) & 0xffff) / 65536.0f - 0.5f) * 1.5f; }
        DevBuf Q((size_t)t * 3 * d, h.data()), O((size_t)t * d);
        unsigned short* img = nullptr;
        WLK_HIP(hipMalloc(reinterpret_cast<void**>(&img), x3_attn_image_elems(t, d) * sizeof(unsigned short)));
        hipStream_t st;
        WLK_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        LaunchCtx ctx{st, nullptr};
        launch_x3_pack_qkv(ctx, Q.p, img, t, d, x3_attn_vt_off(t, d), x3_attn_vt_ld(t));
        auto go = [&]() { launch_encoder_attention_x3(ctx, img, 2L * d, x3_attn_vt_off(t, d), x3_attn_vt_ld(t), O.p, d, t, d, n_head, nullptr, 0); };
        go();
        WLK_HIP(hipStreamSynchronize(st));
        hipEvent_t e0, e1;
        WLK_HIP(hipEventCreate(&e0));
        WLK_HIP(hipEventCreate(&e1));
        WLK_HIP(hipEventRecord(e0, st));
        for (int i = 0; i < reps; ++i) go();
        WLK_HIP(hipEventRecord(e1, st));
        WLK_HIP(hipStreamSynchronize(st));
        float ms = 0.f;
        WLK_HIP(hipEventElapsedTime(&ms, e0, e1));
        *us_per_launch = 1e3f * ms / (float)reps;
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        (void)hipStreamDestroy(st);
        (void)hipFree(img);
    });
}

/* the address sequence of one workgroup of that kernel, from the kernel's own host / device functions (see include/wlk_hip.h);
 * no launch, no device */
int wlk_diag_attn_x3_addresses(int t, int d, int n_head, int head, int q_tile, int64_t* src_off, int32_t* lds_off, int64_t cap,
                               int64_t* n_out, int64_t* image_bytes) {
    try {
        if (!n_out || cap < 0 || (cap > 0 && (!src_off || !lds_off))) throw std::invalid_argument("wlk_diag_attn_x3_addresses: null arguments");
        static_assert(sizeof(long) == sizeof(int64_t) && sizeof(int) == sizeof(int32_t), "address buffers");
        *n_out = enc_attention_x3_addresses(t, d, n_head, head, q_tile, reinterpret_cast<long*>(src_off), reinterpret_cast<int*>(lds_off), (long)cap);
        if (image_bytes) *image_bytes = (int64_t)(x3_attn_image_elems(t, d) * sizeof(unsigned short));
        return WLK_OK;
    } catch (const std::exception& e) {
        g_diag_error = e.what();
        return WLK_ERR_ARG;
    }
}

/* Token selection and AlignAtt read-out (select.hip) on host data through one chosen route: the launchers a decode step
 * uses, unchanged, on caller-chosen logits, adjustments and alignment window (see include/wlk_hip.h) */
int wlk_diag_select(const wlk_diag_select_args* q) {
    std::string bad;
    auto arg_check = [&]() -> bool {
        auto fail = [&](const std::string& m) { bad = "wlk_diag_select: " + m; return false; };
        if (!q) return fail("null arguments");
        if (q->route < 0 || q->route > 4) return fail("route must be 0..4");
        if (q->n_rows < 1 || q->n_rows > 64 || q->n_vocab < 1 || q->k < 1 || q->k > 8) return fail("n_rows in [1, 64], n_vocab >= 1, k in [1, 8]");
        if (!q->logits || !q->top_logprobs || !q->top_ids || !q->frames || !q->attn_last || !q->z || !q->logits_out)
            return fail("null logits / output pointer");
        if (q->n_adj < 0 || (q->n_adj > 0 && (!q->adj_row || !q->adj_ids || !q->adj_deltas))) return fail("bad adjustment triple");
        for (int i = 0; i < q->n_adj; ++i)
            if (q->adj_ids[i] < 0 || q->adj_ids[i] >= q->n_vocab || q->adj_row[i] >= q->n_rows) return fail("adjustment outside the logits");
        if (q->n_align < 1 || q->n_align > 64 || q->T < 1 || q->ring_rows < 1 || !q->ring) return fail("n_align in [1, 64], T >= 1, ring_rows >= 1");
        if (!q->prefill_rows || !q->n_single || !q->newest_row || !q->content_len) return fail("null window counters");
        if (q->single_base < 0) return fail("single_base < 0");
        for (int r = 0; r < q->n_rows; ++r) {
            const int pre = q->prefill_rows[r], ns = q->n_single[r], nw = q->newest_row[r], cl = q->content_len[r];
            if (pre < 0 || ns < 0 || pre + ns < 1 || pre > q->ring_rows || (ns > 0 && q->single_base + ns > q->ring_rows) || nw < 0 ||
                nw >= q->ring_rows || cl < 0 || cl > q->T)
                return fail("window counters of row " + std::to_string(r) + " leave the ring");
            if (q->route != 4 && (pre != q->prefill_rows[0] || ns != q->n_single[0] || nw != q->newest_row[0] || cl != q->content_len[0]))
                return fail("routes 0-3 take one set of window counters and one content_len for all rows");
        }
        if (q->ns_token >= 0 && (q->ns_token >= q->n_vocab || !q->ns_logits || !q->ns_probs)) return fail("bad no-speech request");
        if (q->ns_token >= 0 && q->route == 3) return fail("the early form (route 3) carries no no-speech block");
        if (q->route == 3 && (q->T + 255) / 256 > 64) return fail("the early form (route 3) needs T <= 16384");
        return true;
    };
    if (!arg_check()) {
        g_diag_error = bad;
        return WLK_ERR_ARG;
    }
    bool refused = false;
    const int rc = run([&]() {
        const int R = q->n_rows, V = q->n_vocab, k = q->k, T = q->T, A = q->n_align;
        const bool ns = q->ns_token >= 0;
        struct Stream {
            hipStream_t s = nullptr;
            Stream() { WLK_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); }
            ~Stream() { (void)hipStreamDestroy(s); }
        } st;
        // z carries a guard band on both sides: below T = 4 the read-out kernels form (and discard) median taps whose
        // reflected index lies up to three floats outside the row
        constexpr size_t kGuard = 64;
        const size_t ring_floats = (size_t)A * R * q->ring_rows * T;
        DevBuf L((size_t)R * V, q->logits), NL(ns ? (size_t)R * V : 1, ns ? q->ns_logits : nullptr), NP(R), TV((size_t)R * k),
            RG(ring_floats, q->ring), Z((size_t)R * A * T + 2 * kGuard), AL((size_t)R * T), PT((size_t)R * 64 * 2),
            SC(topk_scratch_bytes(R) / sizeof(float) + 1);
        DevBytes TI((size_t)R * k * sizeof(int)), FR(R * sizeof(int)), AR(q->n_adj * sizeof(int), q->adj_row), AI(q->n_adj * sizeof(int), q->adj_ids);
        DevBuf AD(q->n_adj, q->adj_deltas);
        WLK_HIP(hipMemset(Z.p, 0, ((size_t)R * A * T + 2 * kGuard) * sizeof(float)));
        WLK_HIP(hipMemset(FR.i(), 0xff, R * sizeof(int)));
        WLK_HIP(hipDeviceSynchronize());   // the uploads and fills above ran on the legacy stream; st does not wait for it
        LaunchCtx ctx;
        ctx.stream = st.s;
        AlignArgs a;
        a.ring = RG.p; a.n_align = A; a.n_beam = R; a.ring_rows = q->ring_rows; a.T = T;
        a.prefill_rows = q->prefill_rows[0]; a.n_single = q->n_single[0]; a.newest_row = q->newest_row[0];
        a.single_base = q->single_base; a.content_len = q->content_len[0];
        a.z = Z.p + kGuard; a.attn_last = AL.p; a.frames = FR.i();
        const int *adj_row = q->n_adj ? AR.i() : nullptr, *adj_ids = q->n_adj ? AI.i() : nullptr;
        const float* adj_deltas = q->n_adj ? AD.p : nullptr;
        StepRow* rows_dev = nullptr;
        struct RowsFree {
            StepRow*& p;
            ~RowsFree() { (void)hipFree(p); }
        } rows_free{rows_dev};
        switch (q->route) {
        case 0:
        case 1:
            launch_logsoftmax_topk(ctx, L.p, V, R, k, TV.p, TI.i(), SC.p, adj_row, adj_ids, adj_deltas, q->n_adj);
            if (q->route == 0) {
                launch_alignatt(ctx, a);
            } else {
                launch_align_zscore(ctx, a);
                launch_align_argmax_plain(ctx, a);
            }
            if (ns) launch_token_prob(ctx, NL.p, V, R, q->ns_token, NP.p);
            break;
        case 2:
            refused = !launch_select_fused(ctx, L.p, V, R, k, TV.p, TI.i(), SC.p, adj_row, adj_ids, adj_deltas, q->n_adj, a, StepHostOut{},
                                           ns ? NL.p : nullptr, ns ? q->ns_token : 0, ns ? NP.p : nullptr, false);
            break;
        case 3:
            a.part = PT.p;
            if (!select_fused_applicable(R, k, a)) {
                refused = true;
                break;
            }
            launch_align_zscore(ctx, a);
            refused = !launch_select_fused(ctx, L.p, V, R, k, TV.p, TI.i(), SC.p, adj_row, adj_ids, adj_deltas, q->n_adj, a, StepHostOut{},
                                           nullptr, 0, nullptr, true);
            break;
        default: {
            // row r = a beam-0 session whose window is beam r of the caller's ring: with the ring-row stride of the whole
            // beam group, rows[r].ring + (head * stride) * T lands on ring[head][r][0]
            std::vector<StepRow> rows(R);
            for (int r = 0; r < R; ++r) {
                StepRow sr{};
                sr.ring = RG.p + (size_t)r * q->ring_rows * T;
                sr.prefill_rows = q->prefill_rows[r]; sr.n_single = q->n_single[r]; sr.newest_row = q->newest_row[r];
                sr.content_len = q->content_len[r];
                rows[r] = sr;
            }
            WLK_HIP(hipMalloc(reinterpret_cast<void**>(&rows_dev), sizeof(StepRow) * R));
            WLK_HIP(hipMemcpy(rows_dev, rows.data(), sizeof(StepRow) * R, hipMemcpyHostToDevice));
            a.ring = nullptr;
            a.ring_rows = R * q->ring_rows;
            launch_logsoftmax_topk(ctx, L.p, V, R, k, TV.p, TI.i(), SC.p, adj_row, adj_ids, adj_deltas, q->n_adj);
            launch_alignatt_rows(ctx, a, rows_dev);
            if (ns) launch_token_prob(ctx, NL.p, V, R, q->ns_token, NP.p);
            break;
        }
        }
        WLK_HIP(hipStreamSynchronize(st.s));
        if (refused) return;
        WLK_HIP(hipMemcpy(q->top_logprobs, TV.p, (size_t)R * k * sizeof(float), hipMemcpyDeviceToHost));
        WLK_HIP(hipMemcpy(q->top_ids, TI.i(), (size_t)R * k * sizeof(int), hipMemcpyDeviceToHost));
        WLK_HIP(hipMemcpy(q->frames, FR.i(), (size_t)R * sizeof(int), hipMemcpyDeviceToHost));
        WLK_HIP(hipMemcpy(q->attn_last, AL.p, (size_t)R * T * sizeof(float), hipMemcpyDeviceToHost));
        WLK_HIP(hipMemcpy(q->z, Z.p + kGuard, (size_t)R * A * T * sizeof(float), hipMemcpyDeviceToHost));
        WLK_HIP(hipMemcpy(q->logits_out, L.p, (size_t)R * V * sizeof(float), hipMemcpyDeviceToHost));
        if (ns) WLK_HIP(hipMemcpy(q->ns_probs, NP.p, (size_t)R * sizeof(float), hipMemcpyDeviceToHost));
    });
    if (rc == WLK_OK && refused) {
        g_diag_error = "wlk_diag_select: the fused form does not take this shape (window beyond LDS, or WLK_SELECT_FUSED=0)";
        return WLK_ERR_ARG;
    }
    return rc;
}

/* log_softmax + top-k alone through one chosen form (see include/wlk_hip.h): the launchers a step uses, unchanged */
int wlk_diag_topk(const float* logits, int32_t n_rows, int32_t n_vocab, int32_t k, int32_t form, float* logprobs, int32_t* ids) {
    if (!logits || !logprobs || !ids || n_rows < 1 || n_rows > 64 || n_vocab < 1 || (form != 0 && form != 1)) {
        g_diag_error = "wlk_diag_topk: null pointer, n_rows outside [1, 64], n_vocab < 1 or form not 0 / 1";
        return WLK_ERR_ARG;
    }
    if (k < 1 || k > (form == 0 ? 8 : kTopkWideMaxK)) {
        g_diag_error = "wlk_diag_topk: k must be in [1, 8] (form 0) or [1, 16] (form 1)";
        return WLK_ERR_ARG;
    }
    if (form == 1 && !topk_wide_applicable(n_vocab, k)) {      // (checked here: run() reports what a launcher throws as WLK_ERR_HIP)
        g_diag_error = "wlk_diag_topk: the wide form takes rows of at most 262144 logits";
        return WLK_ERR_ARG;
    }
    return run([&]() {
        struct Stream {
            hipStream_t s = nullptr;
            Stream() { WLK_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); }
            ~Stream() { (void)hipStreamDestroy(s); }
        } st;
        const size_t sc_bytes = form == 0 ? topk_scratch_bytes(n_rows) : topk_wide_scratch_bytes(n_rows);
        DevBuf L((size_t)n_rows * n_vocab, logits), TV((size_t)n_rows * k), TI((size_t)n_rows * k), SC(sc_bytes / sizeof(float) + 1);
        WLK_HIP(hipDeviceSynchronize());   // the uploads ran on the legacy stream; st does not wait for it
        LaunchCtx ctx;
        ctx.stream = st.s;
        int* ti = reinterpret_cast<int*>(TI.p);
        if (form == 0) launch_logsoftmax_topk(ctx, L.p, n_vocab, n_rows, k, TV.p, ti, SC.p, nullptr, nullptr, nullptr, 0);
        else launch_logsoftmax_topk_wide(ctx, L.p, n_vocab, n_rows, k, TV.p, ti, SC.p);
        WLK_HIP(hipStreamSynchronize(st.s));
        WLK_HIP(hipMemcpy(logprobs, TV.p, (size_t)n_rows * k * sizeof(float), hipMemcpyDeviceToHost));
        WLK_HIP(hipMemcpy(ids, ti, (size_t)n_rows * k * sizeof(int), hipMemcpyDeviceToHost));
    });
}

/* the NLLB alignment read-out alone (see include/wlk_hip.h): the launcher an align step uses, unchanged */
int wlk_diag_nllb_align(const float* probs, int32_t n_align, int32_t rows, int32_t S, int32_t lo, int32_t hi, int32_t limit,
                        float* p_out, int32_t* pos, float* prob, float* mass) {
    if (!probs || !p_out || !pos || !prob || !mass || n_align < 1 || n_align > kNlMaxAlign || rows < 1 || rows > 8 || S < 1 ||
        S > kSfMaxFrames) {
        g_diag_error = "wlk_diag_nllb_align: null pointer, n_align outside [1, 64], rows outside [1, 8] or S outside [1, 512]";
        return WLK_ERR_ARG;
    }
    if (lo < 0 || hi > S || limit < 0 || limit > S) {
        g_diag_error = "wlk_diag_nllb_align: needs 0 <= lo, hi <= S and 0 <= limit <= S";
        return WLK_ERR_ARG;
    }
    return run([&]() {
        struct Stream {
            hipStream_t s = nullptr;
            Stream() { WLK_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); }
            ~Stream() { (void)hipStreamDestroy(s); }
        } st;
        const float ctl_host[3] = {__builtin_bit_cast(float, lo), __builtin_bit_cast(float, hi), __builtin_bit_cast(float, limit)};
        DevBuf P((size_t)n_align * rows * S, probs), CTL(3, ctl_host), PO((size_t)rows * S), POS(rows), PR(rows), MS(rows);
        WLK_HIP(hipDeviceSynchronize());   // the uploads ran on the legacy stream; st does not wait for it
        LaunchCtx ctx;
        ctx.stream = st.s;
        launch_nllb_align_readout(ctx, P.p, n_align, rows, S, reinterpret_cast<const int*>(CTL.p), PO.p,
                                  reinterpret_cast<int*>(POS.p), PR.p, MS.p);
        WLK_HIP(hipStreamSynchronize(st.s));
        WLK_HIP(hipMemcpy(p_out, PO.p, (size_t)rows * S * sizeof(float), hipMemcpyDeviceToHost));
        WLK_HIP(hipMemcpy(pos, POS.p, (size_t)rows * sizeof(int), hipMemcpyDeviceToHost));
        WLK_HIP(hipMemcpy(prob, PR.p, (size_t)rows * sizeof(float), hipMemcpyDeviceToHost));
        WLK_HIP(hipMemcpy(mass, MS.p, (size_t)rows * sizeof(float), hipMemcpyDeviceToHost));
    });
}

/* the ragged NLLB alignment read-out alone (see include/wlk_hip.h): the launcher a stacked align step uses, unchanged */
int wlk_diag_nllb_align_rows(const float* probs, int32_t n_align, int32_t rows, int32_t stride, const int32_t* S, const int32_t* lo,
                             const int32_t* hi, const int32_t* limit, float* p_out, int32_t* pos, float* prob, float* mass) {
    if (!probs || !S || !lo || !hi || !limit || !p_out || !pos || !prob || !mass || n_align < 1 || n_align > kNlMaxAlign ||
        rows < 1 || rows > 8 || stride < 1 || stride > kSfMaxFrames) {
        g_diag_error = "wlk_diag_nllb_align_rows: null pointer, n_align outside [1, 64], rows outside [1, 8] or stride outside [1, 512]";
        return WLK_ERR_ARG;
    }
    for (int r = 0; r < rows; ++r) {
        if (S[r] < 1 || S[r] > stride) {
            g_diag_error = "wlk_diag_nllb_align_rows: every S must be in [1, stride]";
            return WLK_ERR_ARG;
        }
        if (lo[r] < 0 || hi[r] > S[r] || limit[r] < 0 || limit[r] > S[r]) {
            g_diag_error = "wlk_diag_nllb_align_rows: needs 0 <= lo, hi <= S and 0 <= limit <= S in every row";
            return WLK_ERR_ARG;
        }
    }
    return run([&]() {
        struct Stream {
            hipStream_t s = nullptr;
            Stream() { WLK_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); }
            ~Stream() { (void)hipStreamDestroy(s); }
        } st;
        StepRow table[8] = {};
        float ctl_host[3 * 8] = {};
        for (int r = 0; r < rows; ++r) {
            table[r].content_len = S[r];
            ctl_host[3 * r] = __builtin_bit_cast(float, lo[r]);
            ctl_host[3 * r + 1] = __builtin_bit_cast(float, hi[r]);
            ctl_host[3 * r + 2] = __builtin_bit_cast(float, limit[r]);
        }
        static_assert(sizeof(StepRow) % sizeof(float) == 0, "the row table is uploaded through a float buffer");
        DevBuf P((size_t)n_align * rows * stride, probs), CTL(3 * 8, ctl_host),
            TB(8 * (sizeof(StepRow) / sizeof(float)), reinterpret_cast<const float*>(table)), PO((size_t)rows * stride), POS(rows), PR(rows),
            MS(rows);
        WLK_HIP(hipDeviceSynchronize());   // the uploads ran on the legacy stream; st does not wait for it
        LaunchCtx ctx;
        ctx.stream = st.s;
        launch_nllb_align_readout_rows(ctx, P.p, n_align, (long)rows * stride, stride, rows, reinterpret_cast<const StepRow*>(TB.p),
                                       reinterpret_cast<const int*>(CTL.p), PO.p, reinterpret_cast<int*>(POS.p), PR.p, MS.p);
        WLK_HIP(hipStreamSynchronize(st.s));
        for (int r = 0; r < rows; ++r)     // only what the kernel wrote: the caller's p_out keeps its fill from S_r on
            WLK_HIP(hipMemcpy(p_out + (size_t)r * stride, PO.p + (size_t)r * stride, (size_t)S[r] * sizeof(float), hipMemcpyDeviceToHost));
        WLK_HIP(hipMemcpy(pos, POS.p, (size_t)rows * sizeof(int), hipMemcpyDeviceToHost));
        WLK_HIP(hipMemcpy(prob, PR.p, (size_t)rows * sizeof(float), hipMemcpyDeviceToHost));
        WLK_HIP(hipMemcpy(mass, MS.p, (size_t)rows * sizeof(float), hipMemcpyDeviceToHost));
    });
}

/* the greedy pick of a draft verification alone (see include/wlk_hip.h): the pick launcher a verify uses, unchanged, and the
 * fold of its slice partials */
int wlk_diag_nllb_verify_pick(const float* logits, int32_t n_rows, int32_t n_vocab, const int32_t* targets, int32_t* picks,
                              int32_t* match) {
    if (!logits || !targets || !picks || !match || n_rows < 1 || n_rows > 128 || n_vocab < 1 || n_vocab > (1 << 20)) {
        g_diag_error = "wlk_diag_nllb_verify_pick: null pointer, n_rows outside [1, 128] or n_vocab outside [1, 2^20]";
        return WLK_ERR_ARG;
    }
    return run([&]() {
        struct Stream {
            hipStream_t s = nullptr;
            Stream() { WLK_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); }
            ~Stream() { (void)hipStreamDestroy(s); }
        } st;
        DevBytes L((size_t)n_rows * n_vocab * sizeof(float), logits), T((size_t)n_rows * sizeof(int), targets),
            PARTS((size_t)n_rows * kNlPickSlices * sizeof(NlPick)), PK((size_t)n_rows * sizeof(int)), MT((size_t)n_rows * sizeof(int));
        WLK_HIP(hipDeviceSynchronize());   // the uploads ran on the legacy stream; st does not wait for it
        LaunchCtx ctx;
        ctx.stream = st.s;
        launch_nllb_verify_pick_rows(ctx, L.f(), n_vocab, n_rows, PARTS.as<NlPick>());
        launch_nllb_verify_fold_rows(ctx, PARTS.as<NlPick>(), n_rows, T.i(), PK.i(), MT.i());
        WLK_HIP(hipStreamSynchronize(st.s));
        PK.back(picks);
        MT.back(match);
    });
}

/* The decoder's attention stage on host data through one chosen route (see include/wlk_hip.h): the launchers of a decode
 * step, unchanged.  Every shape is checked here or by its launcher before anything is launched for it. */
int wlk_diag_dec_attention(const wlk_diag_dec_attention_args* q) {
    struct Refuse : std::invalid_argument {
        using std::invalid_argument::invalid_argument;
    };
    try {
        auto need = [](bool ok, const char* what) {
            if (!ok) throw Refuse(std::string("wlk_diag_dec_attention: ") + what);
        };
        need(q != nullptr, "null arguments");
        const int route = q->route, R = q->n_rows, d = q->d, H = q->n_head, ctx_len = q->ctx_len, T = q->T;
        const bool self_route = route >= WLK_DA_S0 && route <= WLK_DA_S2, cross_route = route >= WLK_DA_C0 && route <= WLK_DA_C5;
        need(self_route || cross_route || (route >= WLK_DA_A0 && route <= WLK_DA_K1), "unknown route");
        need(R >= 1 && R <= 4096, "n_rows in [1, 4096]");
        const float nanf_v = std::nanf("");
        LaunchCtx ctx;
        const size_t F = sizeof(float);

        if (route == WLK_DA_A0) {
            need(ctx_len >= 1 && q->anc && q->anc_rows >= R && q->n_updates >= 0, "A0: a table of at least n_rows rows");
            need(q->n_updates == 0 || (q->ctl && q->upd_offsets), "A0: null update list");
            DevBytes A((size_t)q->anc_rows * ctx_len, q->anc), CT(8 * sizeof(int)), OF(sizeof(int));
            for (int u = 0; u < q->n_updates; ++u) {
                WLK_HIP(hipMemcpy(CT.p, q->ctl + 8 * u, 8 * sizeof(int), hipMemcpyHostToDevice));
                WLK_HIP(hipMemcpy(OF.p, q->upd_offsets + u, sizeof(int), hipMemcpyHostToDevice));
                launch_anc_update(ctx, reinterpret_cast<unsigned char*>(A.p), CT.i(), OF.i(), R, ctx_len);
                WLK_HIP(hipDeviceSynchronize());
            }
            A.back(q->anc);
            return WLK_OK;
        }

        need(d >= 64 && d % 64 == 0 && d <= 4096, "d a multiple of 64 up to 4096");
        if (!cross_route) {
            // ---- self-attention, append, gather: everything over kcache / vcache ------------------------------------
            need(ctx_len >= 1 && ctx_len <= 4096 && q->kcache && q->vcache && q->cache_floats > 0, "a cache and ctx_len in [1, 4096]");
            const size_t row_floats = (size_t)ctx_len * d;
            const long cache_rows = (long)((size_t)q->cache_floats / row_floats);
            const bool rows_form = route == WLK_DA_S1 || route == WLK_DA_K1;
            const long layer_off = rows_form ? q->layer_off : 0;
            need(layer_off >= 0 && layer_off % 4 == 0 && layer_off <= (1 << 24), "layer_off a multiple of 4 in [0, 2^24]");
            const int n_tok = route == WLK_DA_G0 ? 1 : q->n_tok;
            need(n_tok >= 1 && (long)R * n_tok <= 4096, "n_tok >= 1, at most 4096 query rows");
            if (route != WLK_DA_G0) need(q->qkv && q->offsets, "null qkv / offsets");
            if (route == WLK_DA_G0) {
                need(q->n_layer >= 1 && q->row_cache && q->gather_len >= 0 && q->gather_len <= ctx_len &&
                         (long)q->n_layer * R <= cache_rows, "G0: n_layer x n_rows cache rows, gather_len <= ctx_len");
                for (int b = 0; b < R; ++b) need(q->row_cache[b] >= 0 && q->row_cache[b] < R, "G0: source row outside the cache");
            } else if (rows_form) {
                need(n_tok == 1 && q->row_cache, "rows form: one token per row and a cache row per query row");
                for (int r = 0; r < R; ++r)
                    need(q->row_cache[r] >= 0 && q->row_cache[r] < cache_rows && q->offsets[r] >= 0 && q->offsets[r] < ctx_len,
                         "rows form: cache row or offset outside the cache");
            } else {
                need(q->offsets[0] >= 0 && q->offsets[0] + n_tok <= ctx_len && R <= cache_rows, "offset + n_tok <= ctx_len, one cache row per n_rows");
                if (route == WLK_DA_S2) need(n_tok == 1 && q->anc && q->anc_rows >= R, "S2: one token per row and a table of at least n_rows rows");
            }
            const bool attends = self_route;
            if (attends) {
                need(H >= 1 && H * 64 <= d, "64 n_head <= d");
                need(q->out && q->out_floats >= (int64_t)R * n_tok * d, "out holds fewer than the query rows");
            }
            const size_t QR = (size_t)R * n_tok;
            DevBytes QKV(route == WLK_DA_G0 ? 0 : QR * 3 * d * F, q->qkv), KC, VC, OUT(attends ? (size_t)q->out_floats * F : 0, q->out),
                OFF((rows_form ? R : 1) * sizeof(int), route == WLK_DA_G0 ? nullptr : q->offsets), ROWS, ANC, SRC;
            // the caches sit layer_off floats into their allocations; what lies in front of them is NaN
            std::vector<float> front((size_t)layer_off, nanf_v);
            for (DevBytes* c : {&KC, &VC}) {
                c->alloc(((size_t)layer_off + (size_t)q->cache_floats) * F);
                if (layer_off) WLK_HIP(hipMemcpy(c->p, front.data(), (size_t)layer_off * F, hipMemcpyHostToDevice));
                WLK_HIP(hipMemcpy(c->f() + layer_off, c == &KC ? q->kcache : q->vcache, (size_t)q->cache_floats * F, hipMemcpyHostToDevice));
            }
            if (rows_form) {
                std::vector<StepRow> rows(R);
                for (int r = 0; r < R; ++r) {
                    StepRow sr{};
                    sr.kcache = KC.f() + (size_t)q->row_cache[r] * row_floats;
                    sr.vcache = VC.f() + (size_t)q->row_cache[r] * row_floats;
                    sr.offset = q->offsets[r];
                    rows[r] = sr;
                }
                ROWS.alloc(sizeof(StepRow) * R, rows.data());
            }
            if (route == WLK_DA_S2) ANC.alloc((size_t)q->anc_rows * ctx_len, q->anc);
            if (route == WLK_DA_G0) SRC.alloc(R * sizeof(int), q->row_cache);
            WLK_HIP(hipDeviceSynchronize());
            switch (route) {
            case WLK_DA_S0: launch_decoder_self_attention(ctx, QKV.f(), KC.f(), VC.f(), OUT.f(), R, n_tok, OFF.i(), d, H, ctx_len); break;
            case WLK_DA_S1:
                launch_decoder_self_attention_rows(ctx, QKV.f(), reinterpret_cast<const StepRow*>(ROWS.p), layer_off, OUT.f(), R, d, H, ctx_len);
                break;
            case WLK_DA_S2:
                launch_decoder_self_attention_anc(ctx, QKV.f(), KC.f(), VC.f(), reinterpret_cast<const unsigned char*>(ANC.p), OUT.f(), R,
                                                  OFF.i(), d, H, ctx_len);
                break;
            case WLK_DA_G0: launch_kv_gather(ctx, KC.f(), VC.f(), SRC.i(), R, q->gather_len, d, ctx_len, q->n_layer); break;
            case WLK_DA_K0: launch_kv_append(ctx, QKV.f(), KC.f(), VC.f(), R, n_tok, OFF.i(), d, ctx_len); break;
            default: launch_kv_append_rows(ctx, QKV.f(), reinterpret_cast<const StepRow*>(ROWS.p), layer_off, R, d); break;
            }
            WLK_HIP(hipDeviceSynchronize());
            if (attends) {
                OUT.back(q->out);
            } else {
                if (route != WLK_DA_G0) WLK_HIP(hipMemcpy(q->kcache, KC.f() + layer_off, (size_t)q->cache_floats * F, hipMemcpyDeviceToHost));
                WLK_HIP(hipMemcpy(q->vcache, VC.f() + layer_off, (size_t)q->cache_floats * F, hipMemcpyDeviceToHost));
            }
            return WLK_OK;
        }

        // ---- cross-attention ----------------------------------------------------------------------------------------
        need(H >= 1 && H * 64 == d, "cross-attention: d = 64 n_head");
        need(T >= 1 && T <= 8192 && q->k && q->v && q->out, "cross-attention: T in [1, 8192], keys, values, out");
        const bool split_route = route >= WLK_DA_C1 && route <= WLK_DA_C4;
        const int n_kv = route == WLK_DA_C4 ? q->n_kv : 1;
        need(n_kv >= 1 && n_kv <= 8 && (route != WLK_DA_C4 || q->row_kv), "C4: 1..8 key / value sets and row_kv");
        if (split_route) need(R <= 8, "the step forms take at most 8 rows");
        need(route == WLK_DA_C2 ? (q->x && q->wq && q->gamma && q->beta) : q->q != nullptr, "null query operands");
        need(q->out_floats >= (int64_t)R * d, "out holds fewer than n_rows rows");
        const bool align = q->head_rank != nullptr;
        std::vector<int> side_heads, ranks;
        if (align) {
            need(q->n_align >= 1 && q->n_beam >= 1 && q->ring_rows >= 1 && q->ring && q->ring_row && q->beam_of_row, "alignment window missing");
            for (int h = 0; h < H; ++h) {
                need(q->head_rank[h] >= -1 && q->head_rank[h] < q->n_align, "head rank outside the window");
                if (q->head_rank[h] >= 0) { side_heads.push_back(h); ranks.push_back(q->head_rank[h]); }
            }
            for (int r = 0; r < R; ++r)
                need(q->ring_row[r] >= 0 && q->ring_row[r] < q->ring_rows && q->beam_of_row[r] >= 0 && q->beam_of_row[r] < q->n_beam,
                     "ring row or beam outside the window");
        }
        if (route == WLK_DA_C4)
            for (int r = 0; r < R; ++r) need(q->row_kv[r] >= 0 && q->row_kv[r] < n_kv, "C4: key / value set outside k");
        if (route == WLK_DA_C3) {
            need(q->wo && q->bo && q->resid, "C3: null out projection");
            need(gemv1_folds_merge(d), "C3: the out projection does not fold the merge at this width");
        }
        need(route != WLK_DA_C5 || q->k_splits == 0 || q->k_splits == 1, "C5: k_splits is 1 or 0 (the session default)");
        const size_t score_floats = (size_t)R * H * T;
        if (q->scores) need((size_t)q->scores_floats >= score_floats, "scores holds fewer than n_rows x n_head x T floats");

        // keys | values of set s as [T + 1][2][2 d]: layer 0 and row T are NaN
        const long ldkv = 4L * d;
        const size_t set_floats = (size_t)(T + 1) * ldkv;
        std::vector<float> kv(set_floats * n_kv, nanf_v);
        for (int s = 0; s < n_kv; ++s)
            for (int t = 0; t < T; ++t) {
                float* row = kv.data() + s * set_floats + (size_t)t * ldkv + 2 * d;
                memcpy(row, q->k + ((size_t)s * T + t) * d, d * F);
                memcpy(row + d, q->v + ((size_t)s * T + t) * d, d * F);
            }
        const size_t ring_floats = align ? (size_t)q->n_align * q->n_beam * q->ring_rows * T : 0;
        DevBytes KV(kv.size() * F, kv.data()), Q(q->q ? (size_t)R * d * F : 0, q->q), OUT((size_t)q->out_floats * F, q->out),
            RING(ring_floats * F, q->ring), SC(std::max(score_floats, (size_t)(q->scores ? q->scores_floats : 0)) * F, q->scores),
            HR(align ? H * sizeof(int) : 0, q->head_rank), RR(align ? R * sizeof(int) : 0, q->ring_row),
            BR(align ? R * sizeof(int) : 0, q->beam_of_row), SH(side_heads.size() * sizeof(int), side_heads.data()),
            RK(ranks.size() * sizeof(int), ranks.data());
        DevBytes PM((size_t)R * H * kCrossSplitWays * F), PL((size_t)R * H * kCrossSplitWays * F), PO((size_t)R * H * kCrossSplitWays * 64 * F);
        DevBytes X, WQ, BQ, GA, BE, WO, BO, ROWS, PART;
        CrossAttnArgs ca{};
        ca.q = Q.f(); ca.k = KV.f() + 2 * d; ca.v = ca.k + d; ca.ldkv = ldkv; ca.out = OUT.f();
        ca.rows = R; ca.d = d; ca.n_head = H; ca.T = T;
        ca.head_rank = align ? HR.i() : nullptr; ca.ring = align ? RING.f() : nullptr; ca.ring_row = RR.i(); ca.beam_of_row = BR.i();
        ca.ring_rows = q->ring_rows; ca.n_beam = q->n_beam; ca.qk_debug = nullptr; ca.xq_scale = 1.f;
        if (route == WLK_DA_C2) {
            X.alloc((size_t)R * d * F, q->x); WQ.alloc((size_t)d * d * F, q->wq); GA.alloc(d * F, q->gamma); BE.alloc(d * F, q->beta);
            if (q->bq) BQ.alloc(d * F, q->bq);
            ca.q = nullptr;
            ca.xq_x = X.f(); ca.xq_w = WQ.f(); ca.xq_b = q->bq ? BQ.f() : nullptr; ca.xq_gamma = GA.f(); ca.xq_beta = BE.f();
            ca.xq_scale = q->scale;
        }
        if (route == WLK_DA_C4) {
            // row r = a beam-1 session: its keys / values are set row_kv[r], its window is beam beam_of_row[r] of the caller's
            // ring (the ring-row stride of the whole beam group makes rank * stride land on ring[rank][beam][0])
            std::vector<StepRow> rows(R);
            for (int r = 0; r < R; ++r) {
                StepRow sr{};
                sr.cross_kv = KV.f() + (size_t)q->row_kv[r] * set_floats;
                if (align) {
                    sr.ring = RING.f() + (size_t)q->beam_of_row[r] * q->ring_rows * T;
                    sr.ring_row = q->ring_row[r];
                }
                rows[r] = sr;
            }
            ROWS.alloc(sizeof(StepRow) * R, rows.data());
            ca.step_rows = reinterpret_cast<const StepRow*>(ROWS.p);
            ca.kv_off = 2 * d;
            ca.k = nullptr; ca.v = nullptr; ca.ring = nullptr; ca.ring_row = nullptr; ca.beam_of_row = nullptr;
            ca.ring_rows = q->n_beam * q->ring_rows; ca.n_beam = 1;
        }
        WLK_HIP(hipDeviceSynchronize());
        switch (route) {
        case WLK_DA_C0:
            ca.qk_debug = q->scores ? SC.f() : nullptr;
            launch_decoder_cross_attention(ctx, ca);
            break;
        case WLK_DA_C1:
        case WLK_DA_C2:
        case WLK_DA_C4: launch_decoder_cross_attention_split(ctx, ca, SC.f(), PM.f(), PL.f(), PO.f(), true); break;
        case WLK_DA_C3: {
            WO.alloc((size_t)d * d * F, q->wo); BO.alloc(d * F, q->bo);
            WLK_HIP(hipMemcpy(OUT.p, q->resid, d * F, hipMemcpyHostToDevice));      // the residual stream is updated in place
            launch_decoder_cross_attention_split(ctx, ca, SC.f(), PM.f(), PL.f(), PO.f(), false);
            GemmArgs xo;
            xo.mg_pm = PM.f(); xo.mg_pl = PL.f(); xo.mg_po = PO.f(); xo.mg_scores = SC.f();
            xo.mg_head_rank = ca.head_rank; xo.mg_ring = ca.ring; xo.mg_ring_row = ca.ring_row;
            xo.mg_side_heads = align ? SH.i() : nullptr;
            xo.mg_beam_of_row = ca.beam_of_row; xo.mg_heads = H; xo.mg_T = T;
            xo.mg_ring_rows = q->ring_rows; xo.mg_n_beam = q->n_beam;
            xo.mg_side_blocks = align ? (int)side_heads.size() : 0;
            xo.A = Q.f(); xo.lda = d; xo.W = WO.f(); xo.bias = BO.f(); xo.C = OUT.f(); xo.ldc = d; xo.M = R; xo.N = d;
            xo.K = d; xo.flags = kGemmResidual; xo.R = OUT.f(); xo.ldr = d;
            launch_gemv(ctx, xo, "diag_dec_xout");
            break;
        }
        default: {
            FlashArgs fa;
            fa.q = Q.f(); fa.ldq = d; fa.k = ca.k; fa.v = ca.v; fa.ldkv = ldkv; fa.out = OUT.f(); fa.ldo = d;
            fa.Tq = R; fa.Tk = T; fa.n_head = H;
            fa.head_rank = ca.head_rank; fa.ring = ca.ring; fa.ring_row = align ? RR.i() : nullptr;
            fa.beam_of_row = align ? BR.i() : nullptr; fa.ring_rows = q->ring_rows; fa.n_beam = q->n_beam;
            if (q->k_splits == 0) {
                fa.k_splits = wlk_session::flash_splits();
                PART.alloc(flash_split_scratch_floats(R, H, fa.k_splits) * F);
                flash_split_partition(fa, PART.f(), R);
            }
            launch_prefill_cross_attention(ctx, fa);
            // (a session softmaxes every rank behind its last layer; this is one layer, so: the ranks of its heads)
            if (align) launch_ring_softmax(ctx, RING.f(), RR.i(), BR.i(), RK.i(), (int)ranks.size(), R, q->ring_rows, q->n_beam, T);
            break;
        }
        }
        WLK_HIP(hipDeviceSynchronize());
        OUT.back(q->out);
        if (align) RING.back(q->ring);
        if (q->scores) WLK_HIP(hipMemcpy(q->scores, SC.p, (size_t)q->scores_floats * F, hipMemcpyDeviceToHost));
        return WLK_OK;
    } catch (const std::invalid_argument& e) {
        (void)hipDeviceSynchronize();
        g_diag_error = e.what();
        return WLK_ERR_ARG;
    } catch (const std::exception& e) {
        g_diag_error = e.what();
        return WLK_ERR_HIP;
    }
}

/* One kernel of csrc/sortformer.hip on host data through its production launcher (see include/wlk_hip.h).  Every argument is
 * checked here, before anything is uploaded: what reaches a launcher is inside its buffers. */
int wlk_diag_sf_kernel(const wlk_diag_sf_kernel_args* q) {
    struct Refuse : std::invalid_argument {
        using std::invalid_argument::invalid_argument;
    };
    try {
        auto need = [](bool ok, const char* what) {
            if (!ok) throw Refuse(std::string("wlk_diag_sf_kernel: ") + what);
        };
        constexpr size_t kF = sizeof(float);
        need(q != nullptr, "null arguments");
        const int kind = q->kind;
        need(kind >= WLK_SFK_ATTENTION && kind <= WLK_SFK_ASSEMBLE, "unknown kind");
        need(q->out && q->out_floats > 0, "null out");
        LaunchCtx ctx;

        if (kind == WLK_SFK_ATTENTION) {
            const int T = q->T, H = q->n_head, dh = q->dh, n_seg = q->n_seg;
            need(q->form >= 0 && q->form <= 2, "form is 0 (the launcher's rule), 1 (one wave per query) or 2 (matrix cores)");
            need(T >= 1 && T <= kSfMaxFrames, "T in [1, 512]");
            need(dh >= 4 && dh <= 64 && dh % 4 == 0, "dh a multiple of 4 in [4, 64]");
            need(H >= 1 && H <= 64, "n_head in [1, 64]");
            need(n_seg >= 0 && n_seg <= kSfMaxSegments, "n_seg in [0, 8]");
            need(!(q->form == 1 && n_seg > 0), "the one-wave-per-query form does not take segments");
            need(q->q && q->k && q->v, "null q / k / v");
            const long W = (long)H * dh;
            long last = T;          // one past the last row any segment addresses
            if (n_seg > 0) {
                last = 0;
                for (int s = 0; s < n_seg; ++s) {
                    need(q->seg_T[s] >= 1 && q->seg_T[s] <= T, "seg_T in [1, T]");
                    need(q->seg_start[s] >= 0 && q->seg_start[s] <= (1 << 20), "seg_start in [0, 2^20]");
                    last = std::max(last, (long)q->seg_start[s] + q->seg_T[s]);
                }
            }
            auto inside = [&](int64_t ld, int64_t floats, const char* what) {
                need(ld >= W && ld % 4 == 0 && ld <= (1 << 20), what);
                need(floats > 0 && (last - 1) * ld + W <= floats, "a segment lies past a q / k / v / out buffer");
            };
            inside(q->ldq, q->q_floats, "ldq a multiple of 4, at least n_head dh");
            inside(q->ldk, q->k_floats, "ldk a multiple of 4, at least n_head dh");
            inside(q->ldv, q->v_floats, "ldv a multiple of 4, at least n_head dh");
            inside(q->ldo, q->out_floats, "ldo a multiple of 4, at least n_head dh");
            if (q->pos) {
                need(q->pos_row0 >= T - 1, "pos_row0 below T - 1");
                need(q->pos_row0 <= (1 << 20) && q->pos_rows >= 2 * q->pos_row0 + 1, "a pos table has at least 2 pos_row0 + 1 rows");
                need(q->ldp >= W && q->ldp % 4 == 0 && q->ldp <= (1 << 20), "ldp a multiple of 4, at least n_head dh");
                need((int64_t)(q->pos_rows - 1) * q->ldp + W <= q->pos_floats, "the pos table lies past its buffer");
            }
            DevBytes Q, K, V, O, P, U, Vb;
            Q.mirror(q->q, q->q_floats * kF); K.mirror(q->k, q->k_floats * kF); V.mirror(q->v, q->v_floats * kF);
            O.mirror(q->out, q->out_floats * kF);
            if (q->pos) P.mirror(q->pos, q->pos_floats * kF);
            if (q->bias_u) U.alloc(W * kF, q->bias_u);
            if (q->bias_v) Vb.alloc(W * kF, q->bias_v);
            SfAttnArgs a;
            a.q = Q.f(); a.k = K.f(); a.v = V.f(); a.ldq = q->ldq; a.ldk = q->ldk; a.ldv = q->ldv; a.out = O.f(); a.ldo = q->ldo;
            a.T = T; a.n_head = H; a.dh = dh; a.scale = q->scale;
            a.pos = q->pos ? P.f() : nullptr; a.ldp = q->ldp; a.pos_row0 = q->pos_row0;
            a.bias_u = q->bias_u ? U.f() : nullptr; a.bias_v = q->bias_v ? Vb.f() : nullptr;
            a.n_seg = n_seg;
            for (int s = 0; s < n_seg; ++s) { a.seg_start[s] = q->seg_start[s]; a.seg_T[s] = q->seg_T[s]; }
            WLK_HIP(hipDeviceSynchronize());
            launch_sf_attention(ctx, a, q->form);
            WLK_HIP(hipDeviceSynchronize());
            Q.back(); K.back(); V.back(); O.back(); P.back();
            return WLK_OK;
        }

        need(q->in && q->in_floats > 0 && (kind == WLK_SFK_ASSEMBLE || (q->w && q->b)), "null in / w / b");
        if (kind == WLK_SFK_HEAD) {
            const int T = q->T, d = q->d, ns = q->n_spk;
            need(T >= 1 && T <= 4096 && d >= 1 && d <= 4096 && ns >= 1 && ns <= 64, "T in [1, 4096], d in [1, 4096], n_spk in [1, 64]");
            need(q->w2 && q->b2, "null w2 / b2");
            need((int64_t)T * d <= q->in_floats && (int64_t)T * ns <= q->out_floats, "the rows lie past in / out");
            DevBytes X, W1((size_t)d * d * kF, q->w), B1(d * kF, q->b), W2((size_t)ns * d * kF, q->w2), B2(ns * kF, q->b2), O;
            X.mirror(q->in, q->in_floats * kF); O.mirror(q->out, q->out_floats * kF);
            WLK_HIP(hipDeviceSynchronize());
            launch_sf_head(ctx, X.f(), W1.f(), B1.f(), W2.f(), B2.f(), O.f(), T, d, ns);
            WLK_HIP(hipDeviceSynchronize());
            X.back(); O.back();
            return WLK_OK;
        }

        // the stacked kinds: sessions one after the other, tables from the lengths as sf_run_batch builds them
        const int n = q->n_sess;
        need(n >= 1 && n <= kSfMaxSegments, "n_sess in [1, 8]");
        for (int s = 0; s < n; ++s) need(q->len[s] >= (kind == WLK_SFK_ASSEMBLE ? 0 : 1) && q->len[s] <= (1 << 16), "a session length outside [1, 65536]");
        if (kind == WLK_SFK_CONV0 || kind == WLK_SFK_DWCONV2D) {
            const int F = q->F, C = q->C;
            need(F >= 1 && F <= 4096 && C >= 1 && C <= 4096, "F and C in [1, 4096]");
            SfConvSegs sg;
            int f0 = 0, t0 = 0;
            for (int s = 0; s < n; ++s) {
                sg.in_start[sg.n] = f0; sg.in_len[sg.n] = q->len[s]; sg.out_start[sg.n] = t0;
                ++sg.n;
                f0 += q->len[s];
                t0 += sf_sub_len(q->len[s]);
            }
            sg.in_total = f0; sg.out_total = t0;
            const int64_t per_in = kind == WLK_SFK_CONV0 ? F : (int64_t)F * C;
            need(f0 * per_in <= q->in_floats && (int64_t)t0 * sf_sub_len(F) * C <= q->out_floats, "the sessions lie past in / out");
            DevBytes X, Wt((size_t)9 * C * kF, q->w), B(C * kF, q->b), O;
            X.mirror(q->in, q->in_floats * kF); O.mirror(q->out, q->out_floats * kF);
            WLK_HIP(hipDeviceSynchronize());
            if (kind == WLK_SFK_CONV0) launch_sf_conv0(ctx, X.f(), Wt.f(), B.f(), O.f(), sg, F, C);
            else launch_sf_dwconv2d(ctx, X.f(), Wt.f(), B.f(), O.f(), sg, F, C);
            WLK_HIP(hipDeviceSynchronize());
            X.back(); O.back();
            return WLK_OK;
        }
        const int d = q->d;
        need(d >= 1 && d <= 4096, "d in [1, 4096]");
        SfSegments rows, chunks;
        rows.n = chunks.n = n;
        int r0 = 0, c0 = 0;
        for (int s = 0; s < n; ++s) {
            rows.start[s] = r0; rows.len[s] = q->len[s];
            r0 += q->len[s];
        }
        need(r0 >= 1, "no rows");
        if (kind == WLK_SFK_GLU_DWCONV) {
            const int taps = q->taps;
            need(taps >= 1 && taps % 2 == 1 && taps <= 255, "taps odd in [1, 255]");
            need(q->bn_mean && q->bn_invstd && q->bn_w && q->bn_b, "null batch norm");
            need((int64_t)r0 * 2 * d <= q->in_floats && (int64_t)r0 * d <= q->out_floats, "the sessions lie past in / out");
            DevBytes X, Wt((size_t)taps * d * kF, q->w), B(d * kF, q->b), M(d * kF, q->bn_mean), I(d * kF, q->bn_invstd), G(d * kF, q->bn_w),
                Bb(d * kF, q->bn_b), O;
            X.mirror(q->in, q->in_floats * kF); O.mirror(q->out, q->out_floats * kF);
            WLK_HIP(hipDeviceSynchronize());
            launch_sf_glu_dwconv(ctx, X.f(), Wt.f(), B.f(), M.f(), I.f(), G.f(), Bb.f(), O.f(), rows, d, taps);
            WLK_HIP(hipDeviceSynchronize());
            X.back(); O.back();
            return WLK_OK;
        }
        // ASSEMBLE (w / b are not read; in = the context rows at their stacked positions, in2 = the chunk rows)
        need(d % 4 == 0, "d a multiple of 4");
        for (int s = 0; s < n; ++s) {
            need(q->len2[s] >= 0 && q->len2[s] <= q->len[s], "chunk rows in [0, len]");
            chunks.start[s] = c0; chunks.len[s] = q->len2[s];
            c0 += q->len2[s];
        }
        need(c0 == 0 || (q->in2 && (int64_t)c0 * d <= q->in2_floats), "the chunk rows lie past in2");
        need((int64_t)r0 * d <= q->in_floats && (int64_t)r0 * d <= q->out_floats, "the sessions lie past in / out");
        DevBytes X, X2, O;
        X.mirror(q->in, q->in_floats * kF); O.mirror(q->out, q->out_floats * kF);
        if (q->in2 && q->in2_floats > 0) X2.mirror(q->in2, q->in2_floats * kF);
        else X2.alloc(0);
        WLK_HIP(hipDeviceSynchronize());
        launch_sf_assemble(ctx, X.f(), X2.f(), O.f(), rows, chunks, d, q->scale);
        WLK_HIP(hipDeviceSynchronize());
        X.back(); X2.back(); O.back();
        return WLK_OK;
    } catch (const Refuse& e) {
        g_diag_error = e.what();
        return WLK_ERR_ARG;
    } catch (const std::invalid_argument& e) {      // a launcher's own refusal: nothing was launched
        (void)hipDeviceSynchronize();
        g_diag_error = e.what();
        return WLK_ERR_ARG;
    } catch (const std::exception& e) {
        g_diag_error = e.what();
        return WLK_ERR_HIP;
    }
}

/* Routes of wlk_diag_linear_ex and wlk_diag_gemm_plan above 8: 500 + 10 tm + tn, the k-pipe kernel's tile tm x tn through
 * launch_gemm_kp (force_kernel carries the route). */
static const char kRouteRule[] = "route in [0, 8], or 500 + 10 tm + tn for an instantiated k-pipe tile (3x4 3x3 3x2 3x1 2x4 2x2 2x1 4x2)";
static const char kTileShapeRule[] =
    "a k-pipe tile route needs a shape the kp family gives to the k-pipe kernel (k % 128 == 0, k >= 256, m >= 512)";
static bool kp_tile_route(int route) { return route >= 500 && route < 600 && gemm_kpipe_has_tile((route - 500) / 10, (route - 500) % 10); }

/* One linear layer on host data through launch_linear / launch_gemv / launch_gemm / launch_gemm_kp, unchanged (see
 * include/wlk_hip.h).  Everything a kernel of the chosen route may address is checked against the caller's buffer sizes
 * here, before anything is uploaded; the launchers' own refusals follow before anything is launched. */
int wlk_diag_linear_ex(const wlk_diag_linear_args* q) {
    struct Refuse : std::invalid_argument {
        using std::invalid_argument::invalid_argument;
    };
    try {
        auto need = [](bool ok, const char* what) {
            if (!ok) throw Refuse(std::string("wlk_diag_linear_ex: ") + what);
        };
        need(q != nullptr, "null arguments");
        const int route = q->route, M = q->m, N = q->n, K = q->k, batch = q->batch;
        need((route >= 0 && route <= 8) || kp_tile_route(route), kRouteRule);
        need(M >= 1 && M <= (1 << 16) && N >= 1 && N <= (1 << 20) && K >= 1 && K <= (1 << 16), "m in [1, 2^16], n in [1, 2^20], k in [1, 2^16]");
        // a tile probe on a shape the k-pipe kernel of the kp family does not take would run another kernel: refused here
        need(route <= 8 || gemm_kp_takes_kpipe(M, N, K), kTileShapeRule);
        need((q->flags & ~31) == 0, "unknown flag bits");
        need(q->a && q->w && q->c, "null a / w / c");
        need(q->lda >= 1 && q->lda <= (1 << 20) && q->ldc >= N && q->ldc <= (1 << 21), "lda in [1, 2^20], ldc in [n, 2^21]");
        need(batch >= 0 && batch <= kMaxBatch, "batch in [0, 8]");
        need(q->scale_cols >= 0 && q->scale_period >= 0, "scale_cols / scale_period below 0");
        const bool has_res = (q->flags & kGemmResidual) != 0, r_is_c = q->r_is_c != 0;
        const int nz = std::max(batch, 1);
        const int64_t a_span = (int64_t)(M - 1) * q->lda + K, c_span = (int64_t)(M - 1) * q->ldc + N;
        const int64_t ldr = r_is_c ? q->ldc : q->ldr;
        const int64_t r_span = (int64_t)(M - 1) * ldr + N;
        need((int64_t)N * K <= q->w_floats, "w holds fewer than n x k floats");
        need(!q->bias || N <= q->bias_floats, "bias holds fewer than n floats");
        need((q->ln_gamma != nullptr) == (q->ln_beta != nullptr), "ln_gamma and ln_beta come together");
        need(!q->ln_gamma || K <= q->ln_floats, "ln_gamma / ln_beta hold fewer than k floats");
        if (has_res && !r_is_c) need(q->r && ldr >= N && ldr <= (1 << 21), "a residual needs r and ldr in [n, 2^21]");
        need(!r_is_c || has_res, "r_is_c without the residual flag");
        for (int z = 0; z < nz; ++z) {
            const int64_t ao = batch ? q->a_off[z] : 0, co = batch ? q->c_off[z] : 0, ro = batch ? q->r_off[z] : 0;
            need(ao >= 0 && ao % 4 == 0 && ao + a_span <= q->a_floats, "the rows of a lie past its buffer (offsets are multiples of 4)");
            need(co >= 0 && co + c_span <= q->c_floats, "the rows of c lie past its buffer");
            if (has_res && !r_is_c) need(ro >= 0 && ro + r_span <= q->r_floats, "the rows of r lie past its buffer");
        }
        const int kv_mode = q->kv_mode;
        need(kv_mode >= 0 && kv_mode <= 2, "kv_mode is 0, 1 or 2");
        const bool to_gemv = route == 1 || (route == 0 && gemv_applicable(M, K));
        if (kv_mode != 0) {
            need(q->kcache && q->vcache && q->cache_floats > 0, "kv_mode needs kcache / vcache");
            need(q->kv_d >= 1 && N == 3 * q->kv_d, "kv_mode: n = 3 kv_d");
            need(q->kv_ctx >= 1 && q->kv_ctx <= (1 << 16), "kv_ctx in [1, 2^16]");
            need(batch == 0, "kv_mode with batch");
        }
        if (kv_mode == 1) {
            const int ntok = q->kv_ntok;
            need(ntok >= 1 && M % ntok == 0, "kv_ntok >= 1 divides m");
            need(!to_gemv || ntok == 1, "the GEMV kernels append one token per row");
            need(q->kv_pos >= 0 && q->kv_pos + ntok <= q->kv_ctx, "kv_pos + kv_ntok <= kv_ctx");
            need((int64_t)(M / ntok) * q->kv_ctx * q->kv_d <= q->cache_floats, "the caches hold fewer than beams x kv_ctx x kv_d floats");
        }
        if (kv_mode == 2) {
            need(route == 1, "kv_mode 2 (per-row caches) is a launch_gemv operand: route 1");
            need(M <= 8, "kv_mode 2: at most 8 rows");
            need(q->n_caches >= 1 && q->n_caches <= 8 && q->cache_stride >= 1 && q->cache_stride % 4 == 0 &&
                     (int64_t)q->n_caches * q->cache_stride <= q->cache_floats, "n_caches in [1, 8] caches of cache_stride floats inside the buffer");
            need(q->kv_layer_off >= 0 && q->kv_layer_off <= q->cache_stride, "kv_layer_off inside a cache");
            for (int r = 0; r < M; ++r) {
                need(q->kv_row_cache[r] >= 0 && q->kv_row_cache[r] < q->n_caches, "kv_row_cache outside the caches");
                need(q->kv_row_offset[r] >= 0 && q->kv_row_offset[r] < q->kv_ctx &&
                         q->kv_layer_off + ((int64_t)q->kv_row_offset[r] + 1) * q->kv_d <= q->cache_stride, "kv_row_offset outside its cache");
            }
        }

        constexpr size_t kF = sizeof(float);
        DevBytes A, W, B, G, Bt, R, Cc, KC, VC, POS, ROWS;
        A.mirror(q->a, q->a_floats * kF);
        W.mirror(q->w, q->w_floats * kF);
        if (q->bias) B.mirror(q->bias, q->bias_floats * kF);
        if (q->ln_gamma) { G.mirror(q->ln_gamma, q->ln_floats * kF); Bt.mirror(q->ln_beta, q->ln_floats * kF); }
        if (has_res && !r_is_c) R.mirror(q->r, q->r_floats * kF);
        Cc.mirror(q->c, q->c_floats * kF);
        if (kv_mode != 0) { KC.mirror(q->kcache, q->cache_floats * kF); VC.mirror(q->vcache, q->cache_floats * kF); }
        GemmArgs g;
        g.A = A.f(); g.lda = q->lda; g.W = W.f(); g.bias = q->bias ? B.f() : nullptr; g.C = Cc.f(); g.ldc = q->ldc;
        g.R = has_res ? (r_is_c ? Cc.f() : R.f()) : nullptr; g.ldr = ldr;
        g.M = M; g.N = N; g.K = K; g.flags = q->flags; g.scale = q->scale; g.scale_cols = q->scale_cols;
        g.scale_period = q->scale_period;
        g.ln_gamma = q->ln_gamma ? G.f() : nullptr; g.ln_beta = q->ln_gamma ? Bt.f() : nullptr;
        g.batch = batch;
        for (int z = 0; z < batch; ++z) {
            g.z.in[z] = A.f() + q->a_off[z];
            g.z.out[z] = Cc.f() + q->c_off[z];
            g.z.res[z] = has_res ? (r_is_c ? Cc.f() + q->c_off[z] : R.f() + q->r_off[z]) : nullptr;
        }
        for (int z = batch; z < kMaxBatch; ++z) { g.z.in[z] = nullptr; g.z.out[z] = nullptr; g.z.res[z] = nullptr; }
        if (kv_mode == 1) {
            const int pos = (int)q->kv_pos;
            POS.alloc(sizeof(int), &pos);
            g.kcache = KC.f(); g.vcache = VC.f(); g.kv_pos = POS.i();
            g.kv_d = q->kv_d; g.kv_ctx = q->kv_ctx; g.kv_ntok = q->kv_ntok;
        } else if (kv_mode == 2) {
            StepRow table[8] = {};
            for (int r = 0; r < M; ++r) {
                table[r].kcache = KC.f() + (size_t)q->kv_row_cache[r] * q->cache_stride;
                table[r].vcache = VC.f() + (size_t)q->kv_row_cache[r] * q->cache_stride;
                table[r].offset = q->kv_row_offset[r];
            }
            ROWS.alloc(sizeof(table), table);
            g.kv_rows = ROWS.as<const StepRow>();
            g.kv_layer_off = q->kv_layer_off; g.kv_d = q->kv_d; g.kv_ctx = q->kv_ctx;
        }
        g.force_kwave = route == 2;
        g.force_kernel = (route >= 2 && route <= 4) || route >= 6 ? route : 0;      // > 8: the tile probe of launch_gemm_kp
        LaunchCtx ctx;
        WLK_HIP(hipDeviceSynchronize());
        if (route == 0) launch_linear(ctx, g, "diag_linear");
        else if (route == 1) launch_gemv(ctx, g, "diag_gemv");
        else if (route >= 5) launch_gemm_kp(ctx, g, "diag_gemm_kp");
        else launch_gemm(ctx, g, "diag_gemm");
        WLK_HIP(hipDeviceSynchronize());
        A.back(); W.back(); B.back(); G.back(); Bt.back(); R.back(); Cc.back(); KC.back(); VC.back();
        return WLK_OK;
    } catch (const Refuse& e) {
        g_diag_error = e.what();
        return WLK_ERR_ARG;
    } catch (const std::invalid_argument& e) {      // a launcher's own refusal: nothing was launched
        (void)hipDeviceSynchronize();
        g_diag_error = e.what();
        return WLK_ERR_ARG;
    } catch (const std::exception& e) {
        g_diag_error = e.what();
        return WLK_ERR_HIP;
    }
}

int wlk_diag_gemv_variant(int m, int n, int k, int has_ln, int kv_mode, char* out_text, int cap) {
    if (!out_text || cap < 1) return WLK_ERR_ARG;
    // operands that are present are marked by a non-null pointer; gemv_plan dereferences none
    static const float present = 0.f;
    static float cache_present = 0.f;
    GemmArgs g;
    g.A = &present; g.W = &present; g.lda = k; g.M = m; g.N = n; g.K = k;
    if (has_ln) { g.ln_gamma = &present; g.ln_beta = &present; }
    if (kv_mode == 1) { g.kcache = &cache_present; g.vcache = &cache_present; }
    if (kv_mode == 2) g.kv_rows = reinterpret_cast<const StepRow*>(&present);
    char text[160];
    int rc = WLK_OK;
    if (m < 1 || n < 1 || kv_mode < 0 || kv_mode > 2) {
        snprintf(text, sizeof text, "wlk_diag_gemv_variant: m >= 1, n >= 1, kv_mode in [0, 2]");
        rc = WLK_ERR_ARG;
    } else {
        const GemvPlan p = gemv_plan(g);
        if (p.kernel == GemvPlan::kRefused) {
            snprintf(text, sizeof text, "%s", p.refusal);
            rc = WLK_ERR_ARG;
        } else if (p.kernel == GemvPlan::kStaged) {
            snprintf(text, sizeof text, "gemv<%d,%d>", p.width, p.rpw);
        } else if (p.kernel == GemvPlan::kSingleRowMergeLds) {
            snprintf(text, sizeof text, "gemv1_mgl<%d>", p.width);
        } else {
            snprintf(text, sizeof text, "gemv1<%d,%d,%s,%s>", p.width, p.rpw, p.mg ? "mg" : p.ln ? "ln" : "plain", p.full ? "full" : "part");
        }
    }
    if (rc != WLK_OK) g_diag_error = text;
    snprintf(out_text, (size_t)cap, "%s", text);
    return rc;
}

int wlk_diag_gemm_plan(int m, int n, int k, int route, int batch, int has_cache, char* out_text, int cap) {
    if (!out_text || cap < 1) return WLK_ERR_ARG;
    // operands that are present are marked by a non-null pointer; gemm_plan dereferences none
    static const float present = 0.f;
    static float cache_present = 0.f;
    char text[200];
    int rc = WLK_OK;
    const bool tile_route = kp_tile_route(route);
    if (m < 1 || n < 1 || k < 1 || batch < 0 || batch > kMaxBatch) {
        snprintf(text, sizeof text, "wlk_diag_gemm_plan: m >= 1, n >= 1, k >= 1, batch in [0, 8]");
        rc = WLK_ERR_ARG;
    } else if (!((route >= 0 && route <= 8) || tile_route)) {
        snprintf(text, sizeof text, "wlk_diag_gemm_plan: %s", kRouteRule);
        rc = WLK_ERR_ARG;
    } else if (route == 1 || (route == 0 && gemv_applicable(m, k))) {
        snprintf(text, sizeof text, "wlk_diag_gemm_plan: launch_gemv takes this launch (wlk_diag_gemv_variant)");
        rc = WLK_ERR_ARG;
    } else if (tile_route && !gemm_kp_takes_kpipe(m, n, k)) {
        snprintf(text, sizeof text, "wlk_diag_gemm_plan: %s", kTileShapeRule);
        rc = WLK_ERR_ARG;
    } else {
        GemmArgs g;
        g.A = &present; g.W = &present; g.lda = k; g.M = m; g.N = n; g.K = k; g.batch = batch;
        if (has_cache) { g.kcache = &cache_present; g.vcache = &cache_present; }
        g.force_kwave = route == 2;                                                  // (as wlk_diag_linear_ex sets them)
        g.force_kernel = (route >= 2 && route <= 4) || route >= 6 ? route : 0;
        const GemmPlan p = gemm_plan(g, route >= 5);
        switch (p.kernel) {
        case GemmPlan::kRefused: snprintf(text, sizeof text, "%s", p.refusal); rc = WLK_ERR_ARG; break;
        case GemmPlan::kTiled64: snprintf(text, sizeof text, "gemm<64,64>"); break;
        case GemmPlan::kTiled32: snprintf(text, sizeof text, "gemm<32,64>"); break;
        case GemmPlan::kKwave: snprintf(text, sizeof text, "kwave<gemm>"); break;
        case GemmPlan::kKwave16: snprintf(text, sizeof text, "kwave16<gemm>"); break;
        case GemmPlan::kKpKwave2: snprintf(text, sizeof text, "kwave<kp,2>"); break;
        case GemmPlan::kKpKwave1: snprintf(text, sizeof text, "kwave<kp,1>"); break;
        case GemmPlan::kKpKwave16: snprintf(text, sizeof text, "kwave16<kp>"); break;
        case GemmPlan::kKpipe: snprintf(text, sizeof text, "kpipe<%d,%d>", p.tm, p.tn); break;
        }
    }
    if (rc != WLK_OK) g_diag_error = text;
    snprintf(out_text, (size_t)cap, "%s", text);
    return rc;
}

/* One encoder operator on host data through its production launcher, unchanged (see include/wlk_hip.h).  Everything a
 * kernel of the chosen kind may address is checked against the caller's buffer sizes here; what a launcher refuses is
 * decided by the launcher's own check function (x3_gemm_check, layernorm_check, enc_attention_x3_check, x3_pack_check),
 * called here on the same arguments before anything is uploaded, and again by the launcher. */
int wlk_diag_enc_op(const wlk_diag_enc_op_args* q) {
    struct Refuse : std::invalid_argument {
        using std::invalid_argument::invalid_argument;
    };
    try {
        auto need = [](bool ok, const char* what) {
            if (!ok) throw Refuse(std::string("wlk_diag_enc_op: ") + what);
        };
        need(q != nullptr, "null arguments");
        const int kind = q->kind, form = q->form, M = q->m, N = q->n, K = q->k, batch = q->batch;
        need(kind >= WLK_ENC_X3_GEMM && kind <= WLK_ENC_PACK, "kind in [0, 3]");
        need(batch >= 0 && batch <= kMaxBatch, "batch in [0, 8]");
        need(M >= 1 && M <= (1 << 16) && N >= 1 && N <= (1 << 16), "m and n in [1, 2^16]");
        const int nz = std::max(batch, 1);
        const int64_t LD_MAX = 1 << 20;
        auto off = [&](const int64_t (&o)[8], int z) -> int64_t { return batch ? o[z] : 0; };
        // an operand set of `span` elements at o[z], inside `cap` elements, every offset a multiple of `align`
        auto fits = [&](const int64_t (&o)[8], int64_t span, int64_t cap, int align, const char* what) {
            for (int z = 0; z < nz; ++z) need(off(o, z) >= 0 && off(o, z) % align == 0 && off(o, z) + span <= cap, what);
        };
        const bool in_is_x3 = q->in3 != nullptr;
        DevBytes IN, IN3, W, B, R, OUT, OUT3;
        auto upload = [&]() {
            if (q->in) IN.mirror(q->in, q->in_floats * 4);
            if (q->in3) IN3.mirror(q->in3, q->in3_elems * 2);
            if (q->w) W.mirror(q->w, q->w_floats * 4);
            if (q->bias) B.mirror(q->bias, q->bias_floats * 4);
            if (q->r) R.mirror(q->r, q->r_floats * 4);
            if (q->out) OUT.mirror(q->out, q->out_floats * 4);
            if (q->out3) OUT3.mirror(q->out3, q->out3_elems * 2);
        };
        auto download = [&]() { IN.back(); IN3.back(); W.back(); B.back(); R.back(); OUT.back(); OUT3.back(); };
        std::vector<unsigned short*> scratch;      // packed operands (device only)
        struct FreeAll {
            std::vector<unsigned short*>& v;
            ~FreeAll() { for (auto* p : v) (void)hipFree(p); }
        } free_all{scratch};
        auto dev_u16 = [&](size_t n) {
            unsigned short* p = nullptr;
            WLK_HIP(hipMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(n, 32) * sizeof(unsigned short)));
            scratch.push_back(p);
            return p;
        };
        LaunchCtx ctx;
        PtrTable z{};
        if (kind == WLK_ENC_X3_GEMM) {
            need(form >= 0 && form <= 2, "X3_GEMM: form 0 (fp32 rows), 1 (fc1 row image) or 2 (attention operand image)");
            need(K >= 1 && K <= (1 << 16), "k in [1, 2^16]");
            need((q->in != nullptr) != in_is_x3, "X3_GEMM: a is either in (fp32) or in3 (an X3 row image)");
            need(q->w && (int64_t)N * K <= q->w_floats, "w holds fewer than n x k floats");
            need(q->ld_in >= K && q->ld_in <= LD_MAX, "lda in [k, 2^20]");
            need(q->scale_cols >= 0 && q->scale_period >= 0, "scale_cols / scale_period below 0");
            need(q->bias_off >= 0 && (!q->bias || q->bias_off + N <= q->bias_floats), "bias holds fewer than bias_off + n floats");
            const bool has_res = (q->flags & kGemmResidual) != 0, r_is_c = q->r_is_c != 0;
            need(!r_is_c || has_res, "r_is_c without the residual flag");
            const int64_t ldr = r_is_c ? q->ld_out : q->ldr;
            {   // the launcher's own refusals, by the launcher's own function, before anything is uploaded.  Pointers stand in
                // with the alignment the device copies will have: hipMalloc returns 256-byte aligned blocks
                float* const base = reinterpret_cast<float*>(uintptr_t(1) << 20);
                X3GemmArgs t;
                t.lda = q->ld_in; t.bias = q->bias ? base + q->bias_off : nullptr; t.M = M; t.N = N; t.K = K; t.flags = q->flags;
                t.ldc = q->ld_out; t.ldr = ldr; t.batch = batch; t.C = base; t.R = has_res ? base : nullptr;
                t.x3_out = form != 0; t.ldc3 = q->ld_out3; t.vt_col0 = q->vt_col0; t.vt_off = q->vt_off; t.vt_ld = q->vt_ld;
                x3_gemm_check(t);
            }
            if (in_is_x3) fits(q->in3_off, (int64_t)(M - 1) * 3 * q->ld_in + 3 * (int64_t)K, q->in3_elems, 8, "the rows of the X3 a lie past in3 (offsets are multiples of 8)");
            else fits(q->in_off, (int64_t)(M - 1) * q->ld_in + K, q->in_floats, 4, "the rows of a lie past its buffer (offsets are multiples of 4)");
            if (form == 0) {
                need(q->out && q->ld_out >= N && q->ld_out <= LD_MAX, "an fp32 result needs out and ldc in [n, 2^20]");
                fits(q->out_off, (int64_t)(M - 1) * q->ld_out + N, q->out_floats, 4, "the rows of c lie past out (offsets are multiples of 4)");
                if (has_res && !r_is_c) {
                    need(q->r && ldr >= N && ldr <= LD_MAX, "a residual needs r and ldr in [n, 2^20]");
                    fits(q->r_off, (int64_t)(M - 1) * ldr + N, q->r_floats, 4, "the rows of r lie past its buffer (offsets are multiples of 4)");
                }
            } else {
                need(q->out3 != nullptr, "an X3 result needs out3");
                need(q->vt_col0 >= 0 && q->vt_ld <= LD_MAX, "vt_col0 >= 0, vt_ld <= 2^20");
                const int row_cols = std::min(N, q->vt_col0), vt_rows = N - row_cols;
                need(form != 1 || vt_rows == 0, "form 1: vt_col0 >= n (every column goes to the row image)");
                need(q->ld_out3 >= row_cols && q->ld_out3 <= LD_MAX, "ldc3 is at least the row image's columns");
                const int64_t rows_span = row_cols ? (int64_t)(M - 1) * 3 * q->ld_out3 + 3 * (int64_t)row_cols : 0;
                int64_t span = rows_span;
                if (vt_rows > 0) {
                    need(q->vt_off >= rows_span && q->vt_off % 8 == 0, "vt_off lies behind the row image (a multiple of 8)");
                    span = q->vt_off + (int64_t)vt_rows * 3 * q->vt_ld;
                }
                fits(q->out3_off, span, q->out3_elems, 8, "the X3 result lies past out3 (offsets are multiples of 8)");
            }
            upload();
            unsigned short* w3 = dev_u16(x3_w_elems(N, K));
            WLK_HIP(hipDeviceSynchronize());
            launch_x3_pack_w(ctx, W.f(), K, w3, N, K);
            X3GemmArgs g;
            g.lda = q->ld_in; g.W3 = w3; g.bias = q->bias ? B.f() + q->bias_off : nullptr; g.M = M; g.N = N; g.K = K;
            g.flags = q->flags; g.scale = q->scale; g.scale_cols = q->scale_cols; g.scale_period = q->scale_period;
            g.ldc = q->ld_out; g.ldr = ldr; g.batch = batch;
            if (form != 0) {
                g.x3_out = true; g.ldc3 = q->ld_out3; g.vt_col0 = q->vt_col0; g.vt_off = q->vt_off; g.vt_ld = q->vt_ld;
            }
            for (int i = 0; i < nz; ++i) {
                const unsigned short* a3;
                if (in_is_x3) {
                    a3 = IN3.as<unsigned short>() + off(q->in3_off, i);
                } else {
                    unsigned short* p = dev_u16((size_t)M * 3 * q->ld_in);
                    launch_x3_pack(ctx, IN.f() + off(q->in_off, i), q->ld_in, p, q->ld_in, M, K);
                    a3 = p;
                }
                float* c = form == 0 ? OUT.f() + off(q->out_off, i) : reinterpret_cast<float*>(OUT3.as<unsigned short>() + off(q->out3_off, i));
                const float* r = has_res ? (r_is_c ? c : R.f() + off(q->r_off, i)) : nullptr;
                if (batch) {        // exactly run_encode_group's table: in = the X3 image, out = the result (fp32 or X3), res
                    z.in[i] = reinterpret_cast<const float*>(a3); z.out[i] = c; z.res[i] = r;
                } else {
                    g.A3 = a3; g.R = r;
                    if (form == 0) g.C = c;
                    else g.C3 = reinterpret_cast<unsigned short*>(c);
                }
            }
            g.z = z;
            WLK_HIP(hipDeviceSynchronize());
            launch_gemm_x3(ctx, g, "diag_enc_x3_gemm");
        } else if (kind == WLK_ENC_LN) {
            const int d = N;
            need(form == 0 || form == 1, "LN: form 0 (fp32 rows) or 1 (X3 row image)");
            need(q->in && q->w && q->bias, "LN: in, gamma (w) and beta (bias)");
            layernorm_check(d, q->ld_in, q->ld_out3, form == 1, batch);
            need(d <= q->w_floats && d <= q->bias_floats, "gamma / beta hold fewer than d floats");
            need(q->ld_in >= d && q->ld_in <= LD_MAX, "ldx in [d, 2^20]");
            fits(q->in_off, (int64_t)(M - 1) * q->ld_in + d, q->in_floats, form == 1 ? 4 : 1, "the rows of x lie past in");
            if (form == 0) {
                need(q->out && q->ld_out >= d && q->ld_out <= LD_MAX, "an fp32 result needs out and ldy in [d, 2^20]");
                fits(q->out_off, (int64_t)(M - 1) * q->ld_out + d, q->out_floats, 1, "the rows of y lie past out");
            } else {
                need(q->out3 && q->ld_out3 >= d && q->ld_out3 <= LD_MAX, "an X3 result needs out3 and ldy3 in [d, 2^20]");
                fits(q->out3_off, (int64_t)(M - 1) * 3 * q->ld_out3 + 3 * (int64_t)d, q->out3_elems, 8, "the X3 rows of y lie past out3 (offsets are multiples of 8)");
            }
            upload();
            for (int i = 0; i < nz; ++i) {
                z.in[i] = IN.f() + off(q->in_off, i);
                z.out[i] = form == 0 ? OUT.f() + off(q->out_off, i) : reinterpret_cast<float*>(OUT3.as<unsigned short>() + off(q->out3_off, i));
            }
            WLK_HIP(hipDeviceSynchronize());
            if (form == 0 && batch) launch_layernorm_batched(ctx, z, batch, q->ld_in, W.f(), B.f(), q->ld_out, M, d, "diag_enc_ln");
            else if (form == 0) launch_layernorm(ctx, z.in[0], q->ld_in, W.f(), B.f(), z.out[0], q->ld_out, M, d, "diag_enc_ln");
            else if (batch) launch_layernorm_x3_batched(ctx, z, batch, q->ld_in, W.f(), B.f(), q->ld_out3, M, d, "diag_enc_ln_x3");
            else launch_layernorm_x3(ctx, z.in[0], q->ld_in, W.f(), B.f(), reinterpret_cast<unsigned short*>(z.out[0]), q->ld_out3, M, d, "diag_enc_ln_x3");
        } else if (kind == WLK_ENC_ATTENTION) {
            const int T = M, d = N, H = q->n_head;
            need(form == 0 || form == 1, "ATTENTION: form 0 (fp32 kernel) or 1 (X3 kernel)");
            need(H >= 1 && d == 64 * H, "attention: d = 64 n_head");
            const bool x3_out = q->x3_out != 0;
            if (form == 0) {
                need(q->in && !in_is_x3 && !x3_out, "the fp32 attention reads fp32 qkv and writes fp32 rows");
                need(q->out && q->ld_out == d, "the fp32 attention writes rows d apart");
                fits(q->in_off, (int64_t)T * 3 * d, q->in_floats, 4, "qkv [T][3 d] lies past in (offsets are multiples of 4)");
                fits(q->out_off, (int64_t)T * d, q->out_floats, 4, "out [T][d] lies past out (offsets are multiples of 4)");
            } else {
                enc_attention_x3_check(2L * d, x3_attn_vt_ld(T), x3_out ? q->ld_out3 : q->ld_out, T, d, H, x3_out);
                need((q->in != nullptr) != in_is_x3, "ATTENTION: qkv is either in (fp32) or in3 (the X3 operand image)");
                if (in_is_x3) fits(q->in3_off, (int64_t)x3_attn_image_elems(T, d), q->in3_elems, 8, "the operand image lies past in3 (offsets are multiples of 8)");
                else fits(q->in_off, (int64_t)T * 3 * d, q->in_floats, 1, "qkv [T][3 d] lies past in");
                if (x3_out) {
                    need(q->out3 && q->ld_out3 >= d && q->ld_out3 <= LD_MAX, "X3 result rows need out3 and ldo in [d, 2^20]");
                    fits(q->out3_off, (int64_t)(T - 1) * 3 * q->ld_out3 + 3 * (int64_t)d, q->out3_elems, 8, "the X3 rows of out lie past out3 (offsets are multiples of 8)");
                } else {
                    need(q->out && q->ld_out >= d && q->ld_out <= LD_MAX, "an fp32 result needs out and ldo in [d, 2^20]");
                    fits(q->out_off, (int64_t)(T - 1) * q->ld_out + d, q->out_floats, 1, "the rows of out lie past out");
                }
            }
            upload();
            WLK_HIP(hipDeviceSynchronize());
            for (int i = 0; i < nz; ++i) {
                if (form == 0) {
                    z.in[i] = IN.f() + off(q->in_off, i);
                    z.out[i] = OUT.f() + off(q->out_off, i);
                    continue;
                }
                if (in_is_x3) {
                    z.in[i] = reinterpret_cast<const float*>(IN3.as<unsigned short>() + off(q->in3_off, i));
                } else {
                    unsigned short* img = dev_u16(x3_attn_image_elems(T, d));
                    launch_x3_pack_qkv(ctx, IN.f() + off(q->in_off, i), img, T, d, x3_attn_vt_off(T, d), x3_attn_vt_ld(T));
                    z.in[i] = reinterpret_cast<const float*>(img);
                }
                z.out[i] = x3_out ? reinterpret_cast<float*>(OUT3.as<unsigned short>() + off(q->out3_off, i)) : OUT.f() + off(q->out_off, i);
            }
            WLK_HIP(hipDeviceSynchronize());
            if (form == 0 && batch) launch_encoder_attention_batched(ctx, z, batch, T, d, H);
            else if (form == 0) launch_encoder_attention(ctx, z.in[0], z.out[0], T, d, H);
            else
                launch_encoder_attention_x3(ctx, batch ? nullptr : reinterpret_cast<const unsigned short*>(z.in[0]), 2L * d, x3_attn_vt_off(T, d),
                                            x3_attn_vt_ld(T), batch ? nullptr : z.out[0], x3_out ? q->ld_out3 : q->ld_out, T, d, H,
                                            batch ? &z : nullptr, batch, x3_out);
        } else {
            need(batch == 0, "PACK: no batch");
            need(q->in && q->out3, "PACK: in and out3");
            x3_pack_check(q->ld_in, q->ld_out3, N);
            need(q->ld_in >= N && q->ld_in <= LD_MAX && q->ld_out3 >= N && q->ld_out3 <= LD_MAX, "ld_src and ld_dst in [cols, 2^20]");
            need((int64_t)(M - 1) * q->ld_in + N <= q->in_floats, "the rows of src lie past in");
            need((int64_t)(M - 1) * 3 * q->ld_out3 + 3 * (int64_t)N <= q->out3_elems, "the X3 rows lie past out3");
            upload();
            WLK_HIP(hipDeviceSynchronize());
            launch_x3_pack(ctx, IN.f(), q->ld_in, OUT3.as<unsigned short>(), q->ld_out3, M, N);
        }
        WLK_HIP(hipDeviceSynchronize());
        download();
        return WLK_OK;
    } catch (const Refuse& e) {
        g_diag_error = e.what();
        return WLK_ERR_ARG;
    } catch (const std::invalid_argument& e) {      // a launcher's own refusal: nothing was uploaded or launched
        g_diag_error = e.what();
        return WLK_ERR_ARG;
    } catch (const std::exception& e) {
        g_diag_error = e.what();
        return WLK_ERR_HIP;
    }
}

/* The device half of find_alignment behind the vocabulary projection on host data, through launch_word_align, unchanged
 * (see include/wlk_hip.h).  What a buffer cannot hold, and what word_align_check refuses (its own text), is WLK_ERR_ARG
 * before anything is uploaded. */
int wlk_diag_word_align(const wlk_diag_word_align_args* q) {
    struct Refuse : std::invalid_argument {
        using std::invalid_argument::invalid_argument;
    };
    try {
        auto need = [](bool ok, const char* what) {
            if (!ok) throw Refuse(std::string("wlk_diag_word_align: ") + what);
        };
        need(q != nullptr, "null arguments");
        need(q->ring && q->logits && q->targets && q->w && q->probs, "null ring, logits, targets, w or probs");
        const int64_t LIM = 1 << 20;
        need(q->P >= 1 && q->P <= LIM && q->F >= 1 && q->F <= LIM && q->T >= 1 && q->T <= LIM && q->ring_rows >= 1 && q->ring_rows <= LIM &&
                 q->n_align >= 1 && q->n_align <= 64 && q->n_sot >= 0 && q->n_sot <= LIM && q->n_cols >= 1 && q->n_cols <= LIM &&
                 q->ld >= 1 && q->ld <= LIM,
             "P, F, T, ring_rows, n_cols, ld in [1, 2^20], n_align in [1, 64], n_sot in [0, 2^20]");
        const int last = q->last_stage;
        const int64_t n_text = (int64_t)q->P - q->n_sot - 2, N = n_text + 1;
        const int64_t nt = std::max<int64_t>(n_text, 1);
        need(q->targets_n >= nt, "targets holds fewer than n_text entries");
        WordAlignArgs a;
        {   // the launcher's own refusals, by its own function, on stand-in pointers
            float* const base = reinterpret_cast<float*>(uintptr_t(1) << 20);
            a.logits = base; a.ld = q->ld; a.n_cols = q->n_cols; a.target = reinterpret_cast<const int*>(base); a.probs = base;
            a.ring = base; a.ring_rows = q->ring_rows; a.T = q->T; a.n_align = q->n_align; a.P = q->P; a.F = q->F; a.n_sot = q->n_sot;
            a.qk_scale = q->qk_scale; a.w = base; a.cost = q->cost ? base : nullptr;
            a.trace_t = a.trace = q->trace ? reinterpret_cast<signed char*>(base) : nullptr;
            word_align_check(a, q->targets, last);
        }
        need((int64_t)q->n_align * q->ring_rows * q->T <= q->ring_floats, "ring holds fewer than n_align x ring_rows x T floats");
        need((n_text - 1) * q->ld + q->n_cols <= q->logits_floats, "the logit rows lie past their buffer");
        need((int64_t)q->n_align * q->P * q->F <= q->w_floats, "w holds fewer than n_align x P x F floats");
        need(n_text <= q->probs_floats, "probs holds fewer than n_text floats");
        need(last < kWaCost || N * q->F <= q->cost_floats, "cost holds fewer than (n_text + 1) x F floats");
        const int64_t n_trace = (N + 1) * ((int64_t)q->F + 1);
        need(last < kWaDtw || n_trace <= q->trace_bytes, "trace holds fewer than (n_text + 2) x (F + 1) bytes");
        DevBytes RING, LOG, TGT, W, COST, PROBS, TRACE, SCRATCH;
        RING.mirror(q->ring, (size_t)q->ring_floats * 4);
        LOG.mirror(q->logits, (size_t)q->logits_floats * 4);
        TGT.mirror(q->targets, (size_t)q->targets_n * 4);
        W.mirror(q->w, (size_t)q->w_floats * 4);
        PROBS.mirror(q->probs, (size_t)q->probs_floats * 4);
        if (q->cost) COST.mirror(q->cost, (size_t)q->cost_floats * 4);
        if (q->trace) TRACE.mirror(q->trace, (size_t)q->trace_bytes);
        SCRATCH.alloc((size_t)n_trace);
        a.logits = LOG.f(); a.target = reinterpret_cast<const int*>(TGT.p); a.probs = PROBS.f(); a.ring = RING.f(); a.w = W.f();
        a.cost = q->cost ? COST.f() : nullptr;
        a.trace = q->trace ? reinterpret_cast<signed char*>(TRACE.p) : nullptr;
        a.trace_t = q->trace ? reinterpret_cast<signed char*>(SCRATCH.p) : nullptr;
        LaunchCtx ctx;
        WLK_HIP(hipDeviceSynchronize());
        launch_word_align(ctx, a, q->targets, last);
        WLK_HIP(hipDeviceSynchronize());
        RING.back(); LOG.back(); TGT.back(); W.back(); PROBS.back(); COST.back(); TRACE.back();
        return WLK_OK;
    } catch (const std::invalid_argument& e) {      // Refuse, or the launcher's own refusal: nothing was uploaded or launched
        g_diag_error = e.what();
        return WLK_ERR_ARG;
    } catch (const std::exception& e) {
        g_diag_error = e.what();
        return WLK_ERR_HIP;
    }
}

/* The alignment-head survey kernel on host data, through launch_head_survey, unchanged (see include/wlk_hip.h).  What a
 * buffer cannot hold, and what head_survey_check refuses (its own text), is WLK_ERR_ARG before anything is uploaded. */
int wlk_diag_head_survey(const wlk_diag_head_survey_args* q) {
    struct Refuse : std::invalid_argument {
        using std::invalid_argument::invalid_argument;
    };
    try {
        auto need = [](bool ok, const char* what) {
            if (!ok) throw Refuse(std::string("wlk_diag_head_survey: ") + what);
        };
        need(q != nullptr, "null arguments");
        need(q->q && q->k && q->peak, "null q, k or peak");
        const int64_t LIM = 1 << 20;
        need(q->n_layer >= 1 && q->n_layer <= 256 && q->n_head >= 1 && q->n_head <= 256 && q->P >= 1 && q->P <= LIM && q->F >= 1 &&
                 q->F <= LIM && q->Tk >= 1 && q->Tk <= LIM && q->ldq >= 1 && q->ldq <= (LIM << 4) && q->ldkv >= 1 && q->ldkv <= (LIM << 4),
             "n_layer, n_head in [1, 256], P, F, Tk in [1, 2^20], ldq, ldkv in [1, 2^24]");
        need(q->F <= q->Tk, "F beyond the Tk key rows");
        need(q->k_splits >= 0, "negative key split");
        const int64_t d = 64 * (int64_t)q->n_head, rows = (int64_t)q->n_layer * q->n_head * q->P;
        need(q->ldkv >= q->n_layer * 2 * d, "key rows shorter than n_layer x 2 x 64 n_head");
        HeadSurveyArgs a;
        a.ldq = q->ldq; a.q_layer = (long)q->P * q->ldq; a.ldkv = q->ldkv; a.k_layer = 2 * d;
        a.out_head = q->P; a.out_layer = (long)q->n_head * q->P;
        a.n_layer = q->n_layer; a.n_head = q->n_head; a.P = q->P; a.F = q->F; a.k_splits = q->k_splits;
        {   // the launcher's own refusals, by its own function, on stand-in pointers
            float* const base = reinterpret_cast<float*>(uintptr_t(1) << 20);
            a.q = a.k = base; a.peak = a.part = base; a.frame = q->frame ? reinterpret_cast<int*>(base) : nullptr;
            head_survey_check(a);
        }
        need(((int64_t)q->n_layer * q->P - 1) * q->ldq + d <= q->q_floats, "the query rows lie past q");
        need(((int64_t)q->Tk - 1) * q->ldkv + (q->n_layer - 1) * 2 * d + d <= q->k_floats, "the Tk key rows lie past k");
        need(rows <= q->peak_floats, "peak holds fewer than n_layer x n_head x P floats");
        need(!q->frame || rows <= q->frame_n, "frame holds fewer than n_layer x n_head x P entries");
        DevBytes Q, K, PEAK, FRAME, PART;
        Q.mirror(q->q, (size_t)q->q_floats * 4);
        K.mirror(q->k, (size_t)q->k_floats * 4);
        PEAK.mirror(q->peak, (size_t)q->peak_floats * 4);
        if (q->frame) FRAME.mirror(q->frame, (size_t)q->frame_n * 4);
        PART.alloc(head_survey_scratch_floats(a) * 4);
        a.q = Q.f(); a.k = K.f(); a.peak = PEAK.f(); a.frame = q->frame ? FRAME.i() : nullptr; a.part = PART.f();
        LaunchCtx ctx;
        WLK_HIP(hipDeviceSynchronize());
        launch_head_survey(ctx, a);
        WLK_HIP(hipDeviceSynchronize());
        Q.back(); K.back(); PEAK.back(); FRAME.back();
        return WLK_OK;
    } catch (const std::invalid_argument& e) {      // Refuse, or the launcher's own refusal: nothing was uploaded or launched
        g_diag_error = e.what();
        return WLK_ERR_ARG;
    } catch (const std::exception& e) {
        g_diag_error = e.what();
        return WLK_ERR_HIP;
    }
}

int wlk_diag_x3_plan(int m, int n, int k, int batch, int cus, char* out_text, int cap) {
    if (!out_text || cap < 1) return WLK_ERR_ARG;
    char text[256];
    if (m < 1 || n < 1 || k < 64 || k % 64 != 0 || batch < 0 || batch > kMaxBatch || cus < 8) {
        snprintf(text, sizeof text, "wlk_diag_x3_plan: m >= 1, n >= 1, k a multiple of 64, batch in [0, 8], cus >= 8");
        g_diag_error = text;
        snprintf(out_text, (size_t)cap, "%s", text);
        return WLK_ERR_ARG;
    }
    const X3GemmPlan p = x3_gemm_plan(m, n, std::max(batch, 1), cus);
    // the walk of gemm_x3_wide2_kernel, workgroup by workgroup: the tiles it takes and the empty slots between them
    const int band_m = p.banded ? (p.tiles_m + 3) / 4 : p.tiles_m, band_n = p.banded ? (p.tiles_n + 1) / 2 : p.tiles_n;
    const int per_session = band_m * band_n;
    int max_tiles = 0, tiles_total = 0;
    bool skips = false;
    for (int wg = 0; wg < p.blocks; ++wg) {
        const int xcd = p.banded ? wg & 7 : 0, first = p.banded ? wg >> 3 : wg, stride = p.banded ? p.blocks >> 3 : p.blocks;
        const int band_m0 = p.banded ? (xcd >> 1) * band_m : 0, band_n0 = p.banded ? (xcd & 1) * band_n : 0;
        int tiles = 0;
        bool pending_gap = false;
        for (int slot = first; slot < p.slots; slot += stride) {
            const int r = slot % per_session;
            const int rm = p.colmajor ? r % band_m : r / band_n, cn = p.colmajor ? r / band_m : r % band_n;
            if (band_m0 + rm < p.tiles_m && band_n0 + cn < p.tiles_n) {
                if (tiles > 0 && pending_gap) skips = true;
                ++tiles;
                pending_gap = false;
            } else {
                pending_gap = true;
            }
        }
        max_tiles = std::max(max_tiles, tiles);
        tiles_total += tiles;
    }
    snprintf(text, sizeof text, "bm=%d %s %s persist=%d tiles=%dx%d nslab=%d slots=%d blocks=%d walked=%d max_tiles_per_wg=%d skips_between=%d",
             p.bm, p.banded ? "banded" : "plain", p.colmajor ? "colmajor" : "rowmajor", p.persist, p.tiles_m, p.tiles_n, k / 32,
             p.slots, p.blocks, tiles_total, max_tiles, skips ? 1 : 0);
    snprintf(out_text, (size_t)cap, "%s", text);
    return WLK_OK;
}

}  // extern "C"
