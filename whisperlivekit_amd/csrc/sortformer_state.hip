// Device half of the Sortformer streaming state (include/wlk_hip.h, "device-resident diarizer sessions"): the FIFO /
// speaker-cache update and the speaker-cache compression of NeMo's SortformerModules.streaming_update_async /
// _compress_spkcache, for the sessions of one stacked step, after the network.
//
// The spec is the numpy restatement in whisperlivekit_amd/sortformer.py (streaming_update, compress_spkcache), which
// tests/test_sortformer_host.py pins to the oracle.  Every value here is produced by the same fp32 operations in the same
// order (the build has -ffp-contract=off; logf, not __logf; IEEE division):
//   * the silence test is the sequential n_spk-term row sum ((p0 + p1) + p2) + p3 < f32(sil_threshold);
//   * the silence profile is mean * f32(n) + (row_0 * m_0 + row_1 * m_1 + ...), summed from the first popped row with the
//     mask multiplied in (numpy's axis-0 reduction order), divided by f32(max(n, 1));
//   * every top-k orders by (score descending, index ascending) - argsort(-v, kind="stable") - so exact ties (duplicated
//     cache rows, -inf entries, the +inf silence slots) resolve to the lowest index exactly as on the host.
// The top-k passes are rank-by-count over LDS: an entry's rank is the number of entries ahead of it under that key.
// Outputs go to the session's other (ping-pong) buffers, so a step that fails leaves the state it started from intact.
#include "common.h"

namespace wlk {

// ---- FIFO / cache update ---------------------------------------------------------------------------------------
// One workgroup per session.  up_fifo row r (r < f_len + chunk_len) is FIFO row r (activities: the network's fresh ones,
// preds[s_len + r]) or chunk row lc + r - f_len (activities preds[s_len + lc + r]); the first `pop` of them move to the cache.
__global__ __launch_bounds__(256) void sf_state_update_kernel(SfStateBatch b) {
    __shared__ unsigned char sil[kSfStateMaxRows];
    __shared__ int n_sil_s;
    const SfStateJob& j = b.job[blockIdx.x];
    const SfStateParams& p = j.p;
    const int d = p.d, ns = p.n_spk, s_len = j.s_len, f_len = j.f_len, lc = j.lc, pop = j.pop;
    const int new_f = f_len + j.chunk_len;
    auto fifo_row = [&](int r) -> const float* {
        return r < f_len ? j.fifo_in + (long)r * d : j.chunk + (long)(lc + r - f_len) * d;
    };
    auto fifo_pred = [&](int r) -> const float* {
        return r < f_len ? j.preds + (long)(s_len + r) * ns : j.preds + (long)(s_len + lc + r) * ns;
    };
    // silence flags of the popped rows
    for (int r = threadIdx.x; r < pop; r += blockDim.x) {
        const float* pr = fifo_pred(r);
        float s = pr[0];
        for (int k = 1; k < ns; ++k) s = s + pr[k];
        sil[r] = s < p.sil_thr ? 1 : 0;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int n = 0;
        for (int r = 0; r < pop; ++r) n += sil[r];
        n_sil_s = n;
    }
    __syncthreads();
    const int n_sil_old = j.lens_in[2], n_sil = n_sil_s, n_sil_new = n_sil_old + n_sil;
    // silence profile: one thread per embedding column, rows in order
    for (int c = threadIdx.x; c < d; c += blockDim.x) {
        float m = j.mean_in[c];
        if (n_sil > 0) {
            float acc = fifo_row(0)[c] * (sil[0] ? 1.f : 0.f);
            for (int r = 1; r < pop; ++r) acc = acc + fifo_row(r)[c] * (sil[r] ? 1.f : 0.f);
            const float total = m * (float)n_sil_old + acc;
            m = total / (float)max(n_sil_new, 1);
        }
        j.mean_out[c] = m;
    }
    // the FIFO after the pop, zero past its length
    const int f_out = new_f - pop;
    for (long i = threadIdx.x; i < (long)p.F * d; i += blockDim.x) {
        const int r = (int)(i / d), c = (int)(i % d);
        j.fifo_out[i] = r < f_out ? fifo_row(r + pop)[c] : 0.f;
    }
    for (int i = threadIdx.x; i < p.F * ns; i += blockDim.x) {
        const int r = i / ns, k = i % ns;
        j.fifo_p_out[i] = r < f_out ? fifo_pred(r + pop)[k] : 0.f;
    }
    // the cache with the popped rows behind it: into up (N rows, compression follows) or straight into cache_out
    float* ce = j.compress ? j.up : j.cache_out;
    float* cp = j.compress ? j.up_p : j.cache_p_out;
    const int rows = j.compress ? j.N : p.S;
    for (long i = threadIdx.x; i < (long)rows * d; i += blockDim.x) {
        const int t = (int)(i / d), c = (int)(i % d);
        ce[i] = t < s_len ? j.cache_in[(long)t * d + c] : t < s_len + pop ? fifo_row(t - s_len)[c] : 0.f;
    }
    for (int i = threadIdx.x; i < rows * ns; i += blockDim.x) {
        const int t = i / ns, k = i % ns;
        cp[i] = t < s_len ? j.cache_p_in[(long)t * ns + k] : t < s_len + pop ? fifo_pred(t - s_len)[k] : 0.f;
    }
    if (threadIdx.x == 0) {
        j.lens_out[0] = j.compress ? p.S : s_len + pop;
        j.lens_out[1] = f_out;
        j.lens_out[2] = n_sil_new;
    }
}

void launch_sf_state_update(const LaunchCtx& ctx, const SfStateBatch& b) {
    if (b.n <= 0) return;
    if (b.n > kSfMaxSegments) throw std::invalid_argument("sortformer state: too many sessions in one update");
    for (int i = 0; i < b.n; ++i)
        if (b.job[i].f_len + b.job[i].chunk_len > kSfStateMaxRows || b.job[i].pop > b.job[i].f_len + b.job[i].chunk_len)
            throw std::invalid_argument("sortformer state: FIFO rows out of range");
    KernelScope ks(ctx, "sf_state_update");
    hipLaunchKernelGGL(sf_state_update_kernel, dim3(b.n), dim3(256), 0, ctx.stream, b);
    WLK_HIP(hipGetLastError());
}

// ---- compression ------------------------------------------------------------------------------------------------
// One workgroup per compressing session.  sc holds the scores in the flat (speaker, time) order of the global top-k:
// sc[s * nt + t], nt = N + silence slots.
constexpr int kCompressThreads = 512;

// rank of entry i of v[0, n) under (value descending, index ascending): the entries ahead of it
__device__ __forceinline__ int sf_rank_desc(const float* v, int n, int i) {
    const float x = v[i];
    int r = 0;
    for (int k = 0; k < n; ++k) {
        const float y = v[k];
        r += (y > x || (y == x && k < i)) ? 1 : 0;
    }
    return r;
}

__global__ __launch_bounds__(kCompressThreads) void sf_state_compress_kernel(SfStateBatch b) {
    __shared__ float sc[kSfStateMaxKeys];
    __shared__ unsigned char pick[kSfStateMaxKeys];
    __shared__ int sel[kSfMaxFrames], order[kSfMaxFrames];
    __shared__ int n_pos[64];
    // the blockIdx.x-th job with compress != 0
    int ji = 0;
    for (int i = 0, seen = 0; i < b.n; ++i)
        if (b.job[i].compress) {
            if (seen == (int)blockIdx.x) ji = i;
            ++seen;
        }
    const SfStateJob& j = b.job[ji];
    const SfStateParams& p = j.p;
    const int N = j.N, ns = p.n_spk, d = p.d, S = p.S, nt = N + p.sil_per_spk, K = ns * nt;
    if (threadIdx.x < 64) n_pos[threadIdx.x] = 0;
    __syncthreads();
    // _get_log_pred_scores, -inf off speech, the positive count per speaker
    for (int i = threadIdx.x; i < K; i += blockDim.x) {
        const int s = i / nt, t = i % nt;
        float v = INFINITY;                                  // silence slot
        if (t < N) {
            const float* pr = j.up_p + (long)t * ns;
            float rs = logf(fmaxf(1.f - pr[0], p.thr));
            for (int k = 1; k < ns; ++k) rs = rs + logf(fmaxf(1.f - pr[k], p.thr));
            const float ps = pr[s];
            const float lp = logf(fmaxf(ps, p.thr)), l1p = logf(fmaxf(1.f - ps, p.thr));
            v = ps > 0.5f ? ((lp - l1p) + rs) - p.log_half : -INFINITY;
            if (v > 0.f) atomicAdd(&n_pos[s], 1);
        }
        sc[i] = v;
    }
    __syncthreads();
    // _disable_low_scores, the boost of the newest frames
    for (int i = threadIdx.x; i < K; i += blockDim.x) {
        const int s = i / nt, t = i % nt;
        if (t < N) {
            float v = sc[i];
            const bool speech = j.up_p[(long)t * ns + s] > 0.5f;
            if (!(v > 0.f) && speech && n_pos[s] >= p.min_pos) v = -INFINITY;
            if (p.boost_latest > 0.f && t >= S) v = v + p.boost_latest;
            sc[i] = v;
        }
    }
    __syncthreads();
    // _boost_topk_scores: strong pass, then weak pass on the boosted scores; per speaker over the N frame rows
    for (int pass = 0; pass < 2; ++pass) {
        const int k = min(pass == 0 ? p.strong_k : p.weak_k, N);
        const float boost = pass == 0 ? p.strong_boost : p.weak_boost;
        for (int i = threadIdx.x; i < K; i += blockDim.x) {
            const int s = i / nt, t = i % nt;
            pick[i] = (t < N && sf_rank_desc(sc + s * nt, N, t) < k) ? 1 : 0;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < K; i += blockDim.x)
            if (pick[i]) sc[i] = sc[i] - boost;
        __syncthreads();
    }
    // _get_topk_indices: the global top-S over flat (speaker, time) indices; -inf picks -> max_index
    for (int i = threadIdx.x; i < K; i += blockDim.x) {
        const int r = sf_rank_desc(sc, K, i);
        if (r < S) sel[r] = sc[i] != -INFINITY ? i : p.max_index;
    }
    __syncthreads();
    // ascending sort of the picks (equal values: max_index only, interchangeable)
    for (int r = threadIdx.x; r < S; r += blockDim.x) {
        const int v = sel[r];
        int pos = 0;
        for (int q = 0; q < S; ++q) {
            const int w = sel[q];
            pos += (w < v || (w == v && q < r)) ? 1 : 0;
        }
        order[pos] = v;
    }
    __syncthreads();
    // _gather_spkcache_and_preds: disabled slots (max_index, silence slots) take the silence profile and zero activity
    for (long i = threadIdx.x; i < (long)S * d; i += blockDim.x) {
        const int r = (int)(i / d), c = (int)(i % d);
        const int v = order[r];
        const int t = v % nt;
        const bool off = v == p.max_index || t >= N;
        j.cache_out[i] = off ? j.mean_out[c] : j.up[(long)t * d + c];
    }
    for (int i = threadIdx.x; i < S * ns; i += blockDim.x) {
        const int r = i / ns, k = i % ns;
        const int v = order[r];
        const int t = v % nt;
        const bool off = v == p.max_index || t >= N;
        j.cache_p_out[i] = off ? 0.f : j.up_p[(long)t * ns + k];
    }
}

void launch_sf_state_compress(const LaunchCtx& ctx, const SfStateBatch& b) {
    int n = 0;
    for (int i = 0; i < b.n; ++i)
        if (b.job[i].compress) {
            const SfStateParams& p = b.job[i].p;
            if ((b.job[i].N + p.sil_per_spk) * p.n_spk > kSfStateMaxKeys || b.job[i].N < p.S || p.S > kSfMaxFrames ||
                p.n_spk > 64 || p.max_index < 0)
                throw std::invalid_argument("sortformer state: compression geometry out of range");
            ++n;
        }
    if (n == 0) return;
    KernelScope ks(ctx, "sf_state_compress");
    hipLaunchKernelGGL(sf_state_compress_kernel, dim3(n), dim3(kCompressThreads), 0, ctx.stream, b);
    WLK_HIP(hipGetLastError());
}

}  // namespace wlk
