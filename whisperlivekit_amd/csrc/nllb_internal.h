// What nllb.hip (one sentence per session) and nllb_batch.hip (up to 8 sentences per launch chain) share: the model
// handle, the per-layer weight pointers, the error convention of the wlk_nllb_* entry points and the two launcher
// compositions both encoders use.
#pragma once
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/wlk_hip.h"
#include "common.h"

namespace wlk {

inline int nl_fail(int code, const std::string& msg) {
    set_last_error(msg);
    return code;
}
template <typename F>
static int nl_guarded(F&& f) {
    try {
        return f();
    } catch (const HipError& e) {
        return nl_fail(WLK_ERR_HIP, e.what());
    } catch (const std::invalid_argument& e) {
        return nl_fail(WLK_ERR_ARG, e.what());
    } catch (const std::exception& e) {
        return nl_fail(WLK_ERR_STATE, e.what());
    }
}

struct NlSlot {
    std::string name;
    uint64_t offset, numel;
};

struct NlLayer {
    const float *ln1w, *ln1b, *qkvw, *qkvb, *outw, *outb, *lnxw, *lnxb, *xqw, *xqb, *xkvw, *xkvb, *xoutw, *xoutb, *ln2w, *ln2b,
        *fc1w, *fc1b, *fc2w, *fc2b;
};

inline void nl_linear(const LaunchCtx& c, const float* A, long lda, const float* W, const float* b, float* C, long ldc, int M,
                      int N, int K, int flags, const float* R, long ldr, const char* tag, float scale = 1.f, int scale_cols = 0) {
    GemmArgs g;
    g.A = A; g.lda = lda; g.W = W; g.bias = b; g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.K = K;
    g.flags = flags; g.R = R; g.ldr = ldr; g.scale = scale; g.scale_cols = scale_cols;
    launch_linear(c, g, tag);
}

inline void nl_ffn(const LaunchCtx& c, const NlLayer& L, float* x, float* h, float* wide, int R, int d, int f) {
    launch_layernorm(c, x, d, L.ln2w, L.ln2b, h, d, R, d, "nllb_ln2");
    nl_linear(c, h, d, L.fc1w, L.fc1b, wide, f, R, f, d, kGemmRelu, nullptr, 0, "nllb_fc1");
    nl_linear(c, wide, f, L.fc2w, L.fc2b, x, d, R, d, f, kGemmResidual, x, d, "nllb_fc2");
}

// AlignAtt read-out of an NLLB decoder step (nllb.hip): head mean of the selected heads' softmax rows
// probs [n_align][rows][S], its arg-max over [ctl[0], ctl[1]) and its mass from ctl[2] on; ctl, pos, prob and mass may be
// host-coherent memory.  S <= kSfMaxFrames.
constexpr int kNlMaxAlign = 64;
void launch_nllb_align_readout(const LaunchCtx& ctx, const float* probs, int n_align, int rows, int S, const int* ctl,
                               float* p_out, int* pos, float* prob, float* mass);
// The ragged form of a stacked align step (nllb_batch.hip): row r of n_rows (<= 8) has its own length
// rows[r].content_len (<= stride <= 512) and its own window ctl[3 r .. 3 r + 2] = lo | hi | limit; probs
// [n_align][head_stride / stride][stride], p_out [n_rows][stride].  Nothing is read or written at or past a row's length.
void launch_nllb_align_readout_rows(const LaunchCtx& ctx, const float* probs, int n_align, long head_stride, int stride,
                                    int n_rows, const StepRow* rows, const int* ctl, float* p_out, int* pos, float* prob,
                                    float* mass);

}  // namespace wlk

struct wlk_nllb {
    wlk_nllb_dims D{};
    int device = 0;
    float* arena = nullptr;
    uint64_t arena_floats = 0;
    std::vector<wlk::NlSlot> layout;
    std::map<std::string, const wlk::NlSlot*> index;
    bool finalized = false;
    std::vector<wlk::NlLayer> enc, dec;
    const float *emb = nullptr, *pos = nullptr, *enc_lnw = nullptr, *enc_lnb = nullptr, *dec_lnw = nullptr, *dec_lnb = nullptr;
    const float* P(const std::string& n) const {
        auto it = index.find(n);
        if (it == index.end()) throw std::invalid_argument("unknown packed tensor " + n);
        return arena + it->second->offset;
    }
    ~wlk_nllb() {
        (void)hipSetDevice(device);
        if (arena) (void)hipFree(arena);
    }
};
