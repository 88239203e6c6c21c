// Alignment-head survey for checkpoints without a head table (the reference's scripts/determine_alignment_heads.py:125-178,
// `collect_heads`): one teacher-forced decoder pass over [sot sequence, <|notimestamps|>, transcript, <|endoftext|>], and for
// EVERY decoder layer and head the peak of softmax(scores[:, :num_frames // 2]) of every token row.
//
// The peak of a softmax row is 1 / sum_f exp(s_f - max s): the row itself is never needed.  Going through the alignment
// window would take n_layer x n_head x P x 1500 floats (large-v3, P = 448: 1.72 GB) to keep one number per row; the kernel
// below does the QK^T half of flash attention and folds each row online into (max, denominator, arg-max), n_layer x n_head x
// P floats in all.
//
// head_survey_kernel: one 256-thread workgroup = one (layer, head, 32-row query tile, key range).  Operand staging is
// flash_attention_kernel's without the V half: 128 keys per trip through LDS (row stride 68), the four waves take one
// 32-key tile each, S^T[key][q] on v_mfma_f32_32x32x2_f32 (exact fp32 products), so every lane owns one query column and 16
// of the tile's keys.  A lane keeps its own (m, l, frame) over the keys it sees - in ascending order, so a strict `>` keeps
// the lowest index - and the 8 lane states of a query (4 waves x 2 halves) are folded through LDS at the end by the same
// function the cross-workgroup merge uses: the larger m wins, on equal m the lower frame, denominators are rescaled by
// exp(m_s - M).  Keys at or beyond F are never loaded (their staging slots re-read key 0) and never counted.
// Precondition: q and the first F key rows are finite.  Nothing is defined for NaN or infinite scores.
#include <algorithm>
#include <climits>
#include <cmath>
#include <stdexcept>
#include <string>

#include "common.h"
#include "internal.h"
#include "wave_ops.h"

namespace wlk {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kHsQT = 32, kHsKT = 32, kHsWaves = 4, kHsLd = 68;
constexpr int kHsTrip = kHsWaves * kHsKT;      // keys staged per trip

struct SurveyState {
    float m, l;      // running maximum, sum of exp(s - m); (-inf, 0) = no key seen
    int f;           // lowest key index that attains m
};

// The one fold of two partial states (inside a workgroup and across key ranges): the larger m wins, on equal m the lower
// frame; an empty state contributes nothing.
__device__ __forceinline__ SurveyState survey_fold(const SurveyState& a, const SurveyState& b) {
    SurveyState r;
    r.m = fmaxf(a.m, b.m);
    const float fa = a.m == -INFINITY ? 0.f : expf(a.m - r.m);
    const float fb = b.m == -INFINITY ? 0.f : expf(b.m - r.m);
    r.l = a.l * fa + b.l * fb;
    const bool take_b = b.m > a.m || (b.m == a.m && b.f < a.f);
    r.f = take_b ? b.f : a.f;
    return r;
}

__global__ __launch_bounds__(256) void head_survey_kernel(HeadSurveyArgs a) {
    __shared__ __attribute__((aligned(16))) float Ks[kHsWaves * kHsKT * kHsLd];
    __shared__ __attribute__((aligned(16))) float Qs[kHsQT * kHsLd];
    __shared__ float Ms[2 * kHsWaves * kHsQT], Ls[2 * kHsWaves * kHsQT];
    __shared__ int Fs[2 * kHsWaves * kHsQT];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, lq = lane & 31;
    const int F = a.F, P = a.P, n_head = a.n_head;
    const int q_tiles = (P + kHsQT - 1) / kHsQT;
    int b = blockIdx.x;
    const int head = b % n_head;  b /= n_head;
    const int qt = b % q_tiles;   b /= q_tiles;
    const int layer = b % a.n_layer;
    const int ks = b / a.n_layer;
    const int q0 = qt * kHsQT;

    // key range of this workgroup: trips [it_lo, it_hi) of 128 keys (the launcher leaves no range empty)
    const int n_trip_all = (F + kHsTrip - 1) / kHsTrip;
    const int per = (n_trip_all + a.k_splits - 1) / a.k_splits;
    const int it_lo = ks * per;
    const int it_hi = min(n_trip_all, it_lo + per);

    const gcf_ptr kbase = to_global(a.k) + (long)layer * a.k_layer + head * 64;
    float4 rk[8];
    auto fetch = [&](int it) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int idx = tid + 256 * i;
            const int key = it * kHsTrip + (idx >> 4);
            const int c4 = idx & 15;
            rk[i] = ldg4(kbase + (long)(key < F ? key : 0) * a.ldkv + c4 * 4);      // never a row at or beyond F
        }
    };
    fetch(it_lo);
    {   // Q tile -> LDS once; rows at or beyond P are zero
        const float* const aq = a.q + (long)layer * a.q_layer + head * 64;
        float4 qv[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int i = tid + 256 * j, qr = i >> 4, c4 = i & 15;
            qv[j] = *reinterpret_cast<const float4*>(aq + (long)min(q0 + qr, P - 1) * a.ldq + c4 * 4);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int i = tid + 256 * j, qr = i >> 4, c4 = i & 15;
            *reinterpret_cast<float4*>(&Qs[qr * kHsLd + c4 * 4]) = q0 + qr < P ? qv[j] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    const float* Qw = Qs + lq * kHsLd + half * 4;
    const float* Kw = Ks + wave * (kHsKT * kHsLd) + lq * kHsLd + half * 4;

    SurveyState st;
    st.m = -INFINITY; st.l = 0.f; st.f = INT_MAX;
    for (int it = it_lo; it < it_hi; ++it) {
        __syncthreads();      // the previous trip's LDS reads are done
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int idx = tid + 256 * i, kl = idx >> 4, c4 = idx & 15;
            *reinterpret_cast<float4*>(&Ks[kl * kHsLd + c4 * 4]) = rk[i];
        }
        __syncthreads();
        if (it + 1 < it_hi) fetch(it + 1);

        const int key0 = it * kHsTrip + wave * kHsKT;
        if (key0 >= F) continue;      // wave-uniform; the barriers above are reached by every wave of every trip
        f32x16 s;
#pragma unroll
        for (int i = 0; i < 16; ++i) s[i] = 0.f;
        float4 k4 = *reinterpret_cast<const float4*>(Kw);
        float4 q4 = *reinterpret_cast<const float4*>(Qw);
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            s = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.x, q4.x, s, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            float4 kn = k4, qn = q4;
            if (g + 1 < 8) {
                kn = *reinterpret_cast<const float4*>(Kw + (g + 1) * 8);
                qn = *reinterpret_cast<const float4*>(Qw + (g + 1) * 8);
            }
            __builtin_amdgcn_sched_barrier(0);
            s = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.y, q4.y, s, 0, 0, 0);
            s = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.z, q4.z, s, 0, 0, 0);
            s = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.w, q4.w, s, 0, 0, 0);
            k4 = kn;
            q4 = qn;
        }
        // rows of s: key = key0 + (r & 3) + 8 (r >> 2) + 4 half, ascending in r; column: query lq
        float mt = -INFINITY;
        int ft = INT_MAX;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = key0 + (r & 3) + 8 * (r >> 2) + 4 * half;
            if (key >= F) s[r] = -INFINITY;
            if (s[r] > mt) { mt = s[r]; ft = key; }
        }
        if (mt == -INFINITY) continue;      // none of this lane's 16 keys lies below F (no barrier, no MFMA behind this)
        const float m_new = fmaxf(st.m, mt);
        const float alpha = st.m == -INFINITY ? 0.f : expf(st.m - m_new);
        float rs = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) rs += expf(s[r] - m_new);      // exp(-inf) = 0 for the keys at or beyond F
        st.l = st.l * alpha + rs;
        if (mt > st.m) st.f = ft;      // strict: an equal score of a later key keeps the earlier frame
        st.m = m_new;
    }

    // the 8 lane states of every query row (4 waves x 2 halves) -> one
    const int slot = (wave * 2 + half) * kHsQT + lq;
    Ms[slot] = st.m; Ls[slot] = st.l; Fs[slot] = st.f;
    __syncthreads();
    if (tid < kHsQT && q0 + tid < P) {
        SurveyState r;
        r.m = Ms[tid]; r.l = Ls[tid]; r.f = Fs[tid];
#pragma unroll
        for (int j = 1; j < 2 * kHsWaves; ++j) {
            SurveyState o;
            o.m = Ms[j * kHsQT + tid]; o.l = Ls[j * kHsQT + tid]; o.f = Fs[j * kHsQT + tid];
            r = survey_fold(r, o);
        }
        const long row = ((long)layer * n_head + head) * P + q0 + tid;
        if (a.k_splits == 1) {
            a.peak[(long)layer * a.out_layer + (long)head * a.out_head + q0 + tid] = 1.0f / r.l;
            if (a.frame) a.frame[(long)layer * a.out_layer + (long)head * a.out_head + q0 + tid] = r.f;
        } else {      // partial state of this key range: [range][m | l | frame][n_layer n_head P]
            const long n = (long)a.n_layer * n_head * P;
            float* const part = a.part + (long)ks * 3 * n;
            part[row] = r.m;
            part[n + row] = r.l;
            reinterpret_cast<int*>(part)[2 * n + row] = r.f;
        }
    }
}

// folds the k_splits partial states of every (layer, head, token row), in range order
__global__ __launch_bounds__(256) void head_survey_merge_kernel(HeadSurveyArgs a) {
    const long n = (long)a.n_layer * a.n_head * a.P;
    const long row = (long)blockIdx.x * 256 + threadIdx.x;
    if (row >= n) return;
    SurveyState r;
    r.m = a.part[row]; r.l = a.part[n + row]; r.f = reinterpret_cast<const int*>(a.part)[2 * n + row];
    for (int s = 1; s < a.k_splits; ++s) {
        const float* const part = a.part + (long)s * 3 * n;
        SurveyState o;
        o.m = part[row]; o.l = part[n + row]; o.f = reinterpret_cast<const int*>(part)[2 * n + row];
        r = survey_fold(r, o);
    }
    const int p = (int)(row % a.P), head = (int)(row / a.P % a.n_head), layer = (int)(row / a.P / a.n_head);
    const long at = (long)layer * a.out_layer + (long)head * a.out_head + p;
    a.peak[at] = 1.0f / r.l;
    if (a.frame) a.frame[at] = r.f;
}

}  // namespace

void head_survey_check(const HeadSurveyArgs& a) {
    auto need = [](bool ok, const char* what) {
        if (!ok) throw std::invalid_argument(std::string("head survey: ") + what);
    };
    const long LIM = 1 << 20;
    need(a.q && a.k && a.peak, "null q, k or peak");
    need(a.n_layer >= 1 && a.n_layer <= 256 && a.n_head >= 1 && a.n_head <= 256, "n_layer and n_head in [1, 256]");
    need(a.P >= 1 && a.P <= LIM && a.F >= 1 && a.F <= LIM, "P and F in [1, 2^20]");
    const long d = 64L * a.n_head;
    need(a.ldq >= d && a.ldq <= (LIM << 4) && a.ldq % 4 == 0, "query rows at least 64 n_head floats apart, a multiple of 4");
    need(a.ldkv >= d && a.ldkv <= (LIM << 4) && a.ldkv % 4 == 0, "key rows at least 64 n_head floats apart, a multiple of 4");
    need(a.q_layer >= 0 && a.q_layer % 4 == 0 && a.k_layer >= 0 && a.k_layer % 4 == 0, "layer strides of q and k: multiples of 4, not negative");
    need(reinterpret_cast<uintptr_t>(a.q) % 16 == 0 && reinterpret_cast<uintptr_t>(a.k) % 16 == 0, "q and k on 16-byte boundaries");
    need(a.out_head >= a.P && a.out_layer >= (long)a.n_head * a.out_head, "result strides shorter than [n_head][P]");
    need(a.k_splits >= 0, "negative key split");
    const long groups = (long)a.n_layer * a.n_head * ((a.P + kHsQT - 1) / kHsQT) * head_survey_splits(a);
    need(groups <= INT_MAX, "more workgroups than a grid holds");
    need(head_survey_splits(a) == 1 || a.part, "key ranges without their scratch");
}

int head_survey_splits(const HeadSurveyArgs& a) {
    const int n_trip = (a.F + kHsTrip - 1) / kHsTrip;
    int want = a.k_splits;
    if (want <= 0) {      // the launcher's own choice: key ranges only while fewer than 256 workgroups would result
        const long groups = (long)a.n_layer * a.n_head * ((a.P + kHsQT - 1) / kHsQT);
        want = groups >= 256 ? 1 : (int)((256 + groups - 1) / groups);
    }
    want = std::min(want, n_trip);
    const int per = (n_trip + want - 1) / want;      // whole 128-key trips per range, no range empty
    return (n_trip + per - 1) / per;
}

size_t head_survey_scratch_floats(const HeadSurveyArgs& a) {
    const int splits = head_survey_splits(a);
    return splits > 1 ? (size_t)splits * 3 * a.n_layer * a.n_head * a.P : 0;
}

void launch_head_survey(const LaunchCtx& ctx, const HeadSurveyArgs& a) {
    head_survey_check(a);
    HeadSurveyArgs b = a;
    b.k_splits = head_survey_splits(a);
    const long q_tiles = (b.P + kHsQT - 1) / kHsQT;
    const long rows = (long)b.n_layer * b.n_head * b.P;
    // QK^T only: 2 P F 64 flops per head; reads q and the first F keys of every head once, writes two words per row
    KernelScope ks(ctx, "head_survey", 2.0 * rows * (double)b.F * 64.0,
                   4.0 * 64.0 * b.n_layer * b.n_head * ((double)b.P + b.F) + 8.0 * rows);
    hipLaunchKernelGGL(head_survey_kernel, dim3((unsigned)(b.n_layer * b.n_head * q_tiles * b.k_splits)), dim3(256), 0, ctx.stream, b);
    WLK_HIP(hipGetLastError());
    if (b.k_splits > 1) {
        hipLaunchKernelGGL(head_survey_merge_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, ctx.stream, b);
        WLK_HIP(hipGetLastError());
    }
}

}  // namespace wlk

using namespace wlk;

extern "C" {

int wlk_head_survey(wlk_session* s, const int64_t* tokens, int32_t n_tokens, int32_t num_frames, float* peak, int32_t* frame) {
    if (!s || !tokens || !peak) return fail(WLK_ERR_ARG, "NULL argument");
    if (s->beam != 1) return fail(WLK_ERR_ARG, "head_survey needs a beam-1 session");
    if (n_tokens < 1) return fail(WLK_ERR_ARG, "head_survey: n_tokens must be >= 1");
    wlk_model* m = s->m;
    const wlk_dims& D = m->D;
    const int P = n_tokens, F = num_frames / 2;
    if (F < 1 || F > D.n_audio_ctx) return fail(WLK_ERR_ARG, "head_survey: num_frames out of range");
    if (P > D.n_text_ctx) return fail(WLK_ERR_CAPACITY, "head_survey: more tokens than the text context");
    if (!s->encoded) return fail(WLK_ERR_STATE, "head_survey before an encode");
    if (s->engine) return fail(WLK_ERR_STATE, "head_survey: the session is attached to the batch engine");
    if (s->debug || s->prof_on) return fail(WLK_ERR_STATE, "head_survey: not in a debug or profiling session");
    for (int i = 0; i < P; ++i)
        if (tokens[i] < 0 || tokens[i] >= D.n_vocab) return fail(WLK_ERR_ARG, "token id out of range");
    const int d = D.n_text_state, L = D.n_text_layer, H = D.n_text_head;
    HeadSurveyArgs a;
    a.ldq = d; a.q_layer = (long)P * d;
    a.ldkv = (long)L * 2 * d; a.k_layer = 2L * d;
    a.out_head = P; a.out_layer = (long)H * P;
    a.n_layer = L; a.n_head = H; a.P = P; a.F = F;
    const size_t n_q = (size_t)L * P * d, n_out = (size_t)L * H * P, n_part = head_survey_scratch_floats(a);
    int rc = guarded([&]() {
        WLK_HIP(hipSetDevice(m->device));
        // [q of every layer | peak | frame | partial states], grown on demand and kept by the session
        const size_t floats = n_q + 2 * n_out + n_part;
        if (floats > s->survey_cap) {
            WLK_HIP(hipStreamSynchronize(s->stream));
            if (s->survey_buf) WLK_HIP(hipFree(s->survey_buf));
            s->survey_buf = nullptr; s->survey_cap = 0;
            s->survey_buf = dev_alloc<float>(floats);
            s->survey_cap = floats;
        }
        return WLK_OK;
    });
    if (rc != WLK_OK) return rc;
    // the decoder pass: the session's prefill; layer i's scaled cross-attention queries land in slot i of the buffer
    s->survey = true;
    rc = wlk_decode(s, tokens, 1, P, 1, 0);
    s->survey = false;
    if (rc != WLK_OK) return rc;
    return guarded([&]() {
        WLK_HIP(hipSetDevice(m->device));
        a.q = s->survey_buf;
        a.k = s->cross_kv;
        a.peak = s->survey_buf + n_q;
        a.frame = reinterpret_cast<int*>(s->survey_buf + n_q + n_out);
        a.part = s->survey_buf + n_q + 2 * n_out;
        launch_head_survey(s->ctx(), a);
        WLK_HIP(hipStreamSynchronize(s->stream));
        copy_sync(peak, a.peak, n_out * sizeof(float), hipMemcpyDeviceToHost);
        if (frame) copy_sync(frame, a.frame, n_out * sizeof(int), hipMemcpyDeviceToHost);
        // the window no longer holds what the streaming read-out expects: the next decode of this session must be a prefill
        s->n_steps = 0;
        s->self_len = 0;
        return WLK_OK;
    });
}

}  // extern "C"
