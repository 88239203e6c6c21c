// Token selection and AlignAtt read-out - the device half of one decode step's tail:
//   * logit adjustments (suppression = add -inf, DRY penalty = subtract)       a6
//   * log_softmax over the vocabulary + top-k                                   a7
//   * softmax probability of one token (no-speech check)                        a6
//   * AlignAtt: column mean/std over the windowed attention rows -> z-score of the newest row
//     -> width-7 median filter (reflect) -> mean over alignment heads -> arg-max over
//     [0, content_mel_len)                                                      a8
// Reference: whisper/decoding.py:317-338,427-432; simul_whisper/simul_whisper.py:370-437;
// whisper/timing.py:19-54.  Everything here is a small HBM/L2-bound reduction; wavefront
// shuffles do the folding and nothing is copied to the host except k+1 numbers per beam row.
#include <atomic>
#include <cstdlib>

#include "common.h"
#include "wave_ops.h"
#include "align_body.h"

namespace wlk {

constexpr int kSelThreads = 1024;
constexpr int kMaxTopK = 8;

__device__ __forceinline__ float block_max(float v, float* red) {
    v = wave_max(v);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    float r = red[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) r = fmaxf(r, red[w]);
    return r;
}

__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    float r = 0.f;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) r += red[w];
    return r;
}

// log_softmax(x)[i] = (x_i - max) - log(sum exp(x - max)) and top-k, in two stages so the 51864-wide
// row is swept by kSelBlocks workgroups at once: stage 1 leaves per-slice (max, sum exp(x - max_slice),
// k best (value, index)); stage 2 folds the slices.  Ties resolve to the lowest index in both stages.
constexpr int kSelBlocks = 64;
struct SelPartial {
    float mx, sum;
    float v[kMaxTopK];
    int i[kMaxTopK];
};

struct TopkArgs {
    float* logits;
    int n_vocab, k, n_rows;
    SelPartial* parts;
    const int* adj_row;
    const int* adj_ids;
    const float* adj_deltas;
    int n_adj;
    float* top_vals;
    int* top_ids;
    StepHostOut host;   // single-session graph steps: n_adj comes from the device block, results also go to the host
    // first step of an infer: the no-speech probability of the sot rows rides in the second launch (n_rows more blocks)
    const float* ns_logits = nullptr;
    int ns_token = 0;
    float* ns_probs = nullptr;
};

__device__ __forceinline__ void topk_stage1_stream(float* __restrict__ logits, int n_vocab, int k,
                                                 SelPartial* __restrict__ parts, const int* __restrict__ adj_row,
                                                 const int* __restrict__ adj_ids, const float* __restrict__ adj_deltas,
                                                 int n_adj, int slice, int row) {
    __shared__ float red[16];
    __shared__ float cand_v[4];
    __shared__ int cand_i[4];
    __shared__ int taken[kMaxTopK];
    const int tid = threadIdx.x;
    const int per = (n_vocab + kSelBlocks - 1) / kSelBlocks;
    const int lo = slice * per;
    const int hi = min(n_vocab, lo + per);
    float* x = logits + (long)row * n_vocab;
    // logit adjustments that fall into this slice are applied here (each slice is owned by one
    // workgroup, so a workgroup barrier is all the ordering that is needed); ids are unique per row
    for (int i = tid; i < n_adj; i += 256) {
        const int id = adj_ids[i];
        const int r = adj_row[i];
        if (id >= lo && id < hi && (r < 0 || r == row)) x[id] += adj_deltas[i];
    }
    __syncthreads();
    float mx = -INFINITY;
    for (int i = lo + tid; i < hi; i += 256) mx = fmaxf(mx, x[i]);
    mx = block_max(mx, red);
    float sum = 0.f;
    if (mx > -INFINITY)
        for (int i = lo + tid; i < hi; i += 256) sum += expf(x[i] - mx);
    sum = block_sum(sum, red);
    SelPartial* out = parts + (long)row * kSelBlocks + slice;
    if (tid == 0) { out->mx = mx; out->sum = sum; }
    for (int round = 0; round < k; ++round) {
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        for (int i = lo + tid; i < hi; i += 256) {
            bool skip = false;
            for (int t = 0; t < round; ++t) skip |= (taken[t] == i);
            const float v = x[i];
            if (!skip && (v > bv || (v == bv && i < bi))) { bv = v; bi = i; }
        }
        wave_argmax(bv, bi);
        __syncthreads();
        if ((tid & 63) == 0) { cand_v[tid >> 6] = bv; cand_i[tid >> 6] = bi; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < 4; ++w)
                if (cand_v[w] > bv || (cand_v[w] == bv && cand_i[w] < bi)) { bv = cand_v[w]; bi = cand_i[w]; }
            taken[round] = bi;
            out->v[round] = bv;
            out->i[round] = bi;
        }
        __syncthreads();
    }
}

// The same slice pass with the slice held in registers (slices of up to 1024 logits: every Whisper vocabulary): ONE read
// of the row instead of k + 2 passes over it (each pass of the streaming form is a memory round trip on a kernel that
// starts with a cold L2), the logit adjustments ride through LDS to the thread that owns the element, and the
// wave-level folds are VALU butterflies (wave_ops.h).  Max, exp-sum (same per-thread order: ascending index) and the
// index-tie-broken arg-max rounds give what the streaming form gives, bit for bit.
constexpr int kSelKeep = 4;
__device__ __forceinline__ void topk_stage1_body(float* __restrict__ logits, int n_vocab, int k,
                                                 SelPartial* __restrict__ parts, const int* __restrict__ adj_row,
                                                 const int* __restrict__ adj_ids, const float* __restrict__ adj_deltas,
                                                 int n_adj, int slice, int row) {
    const int per = (n_vocab + kSelBlocks - 1) / kSelBlocks;
    if (per > 256 * kSelKeep) {
        topk_stage1_stream(logits, n_vocab, k, parts, adj_row, adj_ids, adj_deltas, n_adj, slice, row);
        return;
    }
    __shared__ float red[16];
    __shared__ float cand_v[4];
    __shared__ int cand_i[4];
    __shared__ float adj_buf[256 * kSelKeep];
    const int tid = threadIdx.x;
    const int lo = slice * per;
    const int hi = min(n_vocab, lo + per);
    float* x = logits + (long)row * n_vocab;
    float xv[kSelKeep];
    // (an EMPTY trailing slice - 63 * ceil(V / 64) >= V, i.e. vocabularies below ~4000 tokens - has lo >= n_vocab: the
    // fallback element is clamped into the row so nothing is read behind it; its lanes all take the i >= hi path below)
    const int lo_safe = lo < n_vocab ? lo : n_vocab - 1;
#pragma unroll
    for (int j = 0; j < kSelKeep; ++j) {
        const int i = lo + tid + 256 * j;
        xv[j] = x[i < hi ? i : lo_safe];
        adj_buf[tid + 256 * j] = 0.f;
    }
    __syncthreads();
    // adjustments that fall into this slice (ids are unique per row): delivered to the owner of the element; a thread's
    // three operands are requested together (clamped index), not one dependent load after the other
    for (int i0 = 0; i0 < n_adj; i0 += 256) {
        const int i = i0 + tid, ic = i < n_adj ? i : 0;
        const int id = adj_ids[ic];
        const int r = adj_row[ic];
        const float dl = adj_deltas[ic];
        if (i < n_adj && id >= lo && id < hi && (r < 0 || r == row)) adj_buf[id - lo] = dl;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kSelKeep; ++j) {
        const int i = lo + tid + 256 * j;
        const float a = adj_buf[tid + 256 * j];
        if (a != 0.f && i < hi) {
            xv[j] += a;
            x[i] = xv[j];          // the row stays adjusted in memory, as wlk_select's contract says
        }
    }
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < kSelKeep; ++j)
        if (lo + tid + 256 * j < hi) mx = fmaxf(mx, xv[j]);
    mx = block_max(mx, red);
    float sum = 0.f;
    if (mx > -INFINITY) {
#pragma unroll
        for (int j = 0; j < kSelKeep; ++j)
            if (lo + tid + 256 * j < hi) sum += expf(xv[j] - mx);
    }
    sum = block_sum(sum, red);
    SelPartial* out = parts + (long)row * kSelBlocks + slice;
    if (tid == 0) { out->mx = mx; out->sum = sum; }
    int taken = -1;                      // round r skips what rounds < r took: every thread tracks the winners itself
    int taken_all[kMaxTopK];
#pragma unroll
    for (int t = 0; t < kMaxTopK; ++t) taken_all[t] = -1;
    for (int round = 0; round < k; ++round) {
        float bv = -INFINITY;
        int bi = 0x7fffffff;
#pragma unroll
        for (int j = 0; j < kSelKeep; ++j) {
            const int i = lo + tid + 256 * j;
            if (i < hi) {
                bool skip = false;
#pragma unroll
                for (int t = 0; t < kMaxTopK; ++t) skip |= (t < round && taken_all[t] == i);
                const float v = xv[j];
                if (!skip && (v > bv || (v == bv && i < bi))) { bv = v; bi = i; }
            }
        }
        wave_argmax(bv, bi);
        __syncthreads();
        if ((tid & 63) == 0) { cand_v[tid >> 6] = bv; cand_i[tid >> 6] = bi; }
        __syncthreads();
        bv = cand_v[0];
        bi = cand_i[0];
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (cand_v[w] > bv || (cand_v[w] == bv && cand_i[w] < bi)) { bv = cand_v[w]; bi = cand_i[w]; }
        taken = bi;
#pragma unroll
        for (int t = 0; t < kMaxTopK; ++t)
            if (t == round) taken_all[t] = taken;
        if (tid == 0) {
            out->v[round] = bv;
            out->i[round] = bi;
        }
    }
}

__global__ __launch_bounds__(256) void topk_stage1_kernel(float* __restrict__ logits, int n_vocab, int k,
                                                          SelPartial* __restrict__ parts, const int* __restrict__ adj_row,
                                                          const int* __restrict__ adj_ids,
                                                          const float* __restrict__ adj_deltas, int n_adj) {
    topk_stage1_body(logits, n_vocab, k, parts, adj_row, adj_ids, adj_deltas, n_adj, blockIdx.x, blockIdx.y);
}

// results of a single-session graph step go straight into pinned host memory; the flag is stored after a system-scope
// fence, so a host that sees the flag sees the fields
__device__ __forceinline__ void publish_flag(unsigned* flag, unsigned seq) {
    __threadfence_system();
    __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

__device__ __forceinline__ void topk_stage2_body(const SelPartial* __restrict__ parts, int k,
                                                 float* __restrict__ top_vals, int* __restrict__ top_ids, int row,
                                                 const StepHostOut host = StepHostOut{}, unsigned seq = 0,
                                                 const bool publish = true) {
    const int lane = threadIdx.x;   // one lane per slice (the first wave of the workgroup)
    const SelPartial p = parts[(long)row * kSelBlocks + lane];
    float mx = wave_max(p.mx);
    asm volatile("" : "+v"(seq));   // requested with the partials, not in front of the flag store at the very end
    float sum = p.mx > -INFINITY ? p.sum * expf(p.mx - mx) : 0.f;
    sum = wave_sum(sum);
    const float lse = logf(sum);
    int head = 0;                   // next unconsumed candidate of this slice (its list is sorted)
    for (int round = 0; round < k; ++round) {
        float bv = head < k ? p.v[0] : -INFINITY;
        int bi = head < k ? p.i[0] : 0x7fffffff;
#pragma unroll
        for (int t = 1; t < kMaxTopK; ++t)
            if (t == head && t < k) { bv = p.v[t]; bi = p.i[t]; }
        if (head >= k) { bv = -INFINITY; bi = 0x7fffffff; }
        float wv = bv;
        int wi = bi;
        wave_argmax(wv, wi);
        if (wi == bi && bi != 0x7fffffff) ++head;
        if (lane == 0) {
            top_ids[row * k + round] = wi;
            top_vals[row * k + round] = (wv - mx) - lse;
            if (host.result && round < 2) {
                host.result[row].top_ids[round] = wi;
                host.result[row].top_vals[round] = (wv - mx) - lse;
            }
        }
    }
    if (publish && host.result && lane == 0) publish_flag(&host.result[row].flag_topk, seq);
}

__global__ __launch_bounds__(64) void topk_stage2_kernel(const SelPartial* __restrict__ parts, int k,
                                                         float* __restrict__ top_vals, int* __restrict__ top_ids) {
    topk_stage2_body(parts, k, top_vals, top_ids, blockIdx.x);
}

void launch_logsoftmax_topk(const LaunchCtx& ctx, float* logits, int n_vocab, int n_rows, int k,
                            float* top_vals, int* top_ids, void* scratch, const int* adj_row, const int* adj_ids,
                            const float* adj_deltas, int n_adj) {
    if (k < 1 || k > kMaxTopK) throw std::invalid_argument("top-k: k must be in [1, 8]");
    SelPartial* parts = static_cast<SelPartial*>(scratch);
    {
        KernelScope ks(ctx, "sel_topk_stage1", 0.0, 4.0 * 3.0 * n_rows * (double)n_vocab);
        hipLaunchKernelGGL(topk_stage1_kernel, dim3(kSelBlocks, n_rows), dim3(256), 0, ctx.stream, logits, n_vocab, k,
                           parts, adj_row, adj_ids, adj_deltas, n_adj);
        WLK_HIP(hipGetLastError());
    }
    {
        KernelScope ks(ctx, "sel_topk_stage2");
        hipLaunchKernelGGL(topk_stage2_kernel, dim3(n_rows), dim3(64), 0, ctx.stream, parts, k, top_vals, top_ids);
        WLK_HIP(hipGetLastError());
    }
}

size_t topk_scratch_bytes(int n_rows) { return sizeof(SelPartial) * kSelBlocks * (size_t)n_rows; }

// ---------------------------------------------------------------------------------------------
// The wide form: log_softmax + the k <= 16 best of rows of up to 262 144 logits - what a beam search over
// NLLB's 256 206-token vocabulary asks for (2 n continuations per row, n <= 8).  Same partition as above (64 slices per
// row, thread tid of a slice owns lo + tid + 256 j) and the same order of every max / exp-sum, so the (max, sum) of a slice,
// the row's normaliser and therefore ranks 0..7 are bit for bit those of the forms above; no adjustment list.
//   * the slice lives in registers, 16 entries per thread, all 16 loads issued before the first use: ONE read of the row
//     where topk_stage1_stream (which every NLLB-wide row takes above) makes k + 2 passes.  A lane past `hi` loads a
//     clamped in-row address and holds -inf.
//   * the k best of the slice by (value descending, index ascending) in k exclusion rounds, rules_topk_body's scheme: every
//     thread holds the best entry it has left, a round is one wave_argmax + a 4-entry fold through LDS, and only the thread
//     that owned the winner rescans its 16 registers for what comes after it.  -inf entries are never candidates: a slice
//     with fewer than k finite entries ends its list with (-inf, none).
//   * stage 2, one wave per row, lane = slice: the 64 sorted lists sit in LDS as [position][lane] (a lane only ever reads
//     its own column: no barrier, no bank conflict) and each lane holds the head of its list in registers; a round is one
//     wave_argmax, and the lane that owned the winner fetches its next entry.  Rows with fewer than k finite entries
//     fill up with (-inf, -1).
// ---------------------------------------------------------------------------------------------
constexpr int kWideTopK = kTopkWideMaxK;
constexpr int kWideKeep = 16;
static_assert(kTopkWideMaxVocab == kSelBlocks * 256 * kWideKeep, "the wide form's width limit is its register tile");
constexpr int kWideNone = 0x7fffffff;
struct WidePartial {
    float mx, sum;
    float v[kWideTopK];
    int i[kWideTopK];
};

__global__ __launch_bounds__(256) void topk_wide_stage1_kernel(const float* __restrict__ logits, int n_vocab, int k,
                                                               WidePartial* __restrict__ parts) {
    __shared__ float red[16];
    __shared__ float cand_v[4];
    __shared__ int cand_i[4];
    const int tid = threadIdx.x, slice = blockIdx.x, row = blockIdx.y;
    const int per = (n_vocab + kSelBlocks - 1) / kSelBlocks;
    const int lo = slice * per;
    const int hi = min(n_vocab, lo + per);
    const float* x = logits + (long)row * n_vocab;
    // (an empty trailing slice has lo >= n_vocab: the fallback element is clamped into the row, as in topk_stage1_body)
    const int lo_safe = lo < n_vocab ? lo : n_vocab - 1;
    float xv[kWideKeep];
#pragma unroll
    for (int j = 0; j < kWideKeep; ++j) {
        const int i = lo + tid + 256 * j;
        xv[j] = x[i < hi ? i : lo_safe];
    }
#pragma unroll
    for (int j = 0; j < kWideKeep; ++j) pin_loaded(xv[j]);
    __builtin_amdgcn_sched_barrier(0);     // all 16 requests are out before the first wait
#pragma unroll
    for (int j = 0; j < kWideKeep; ++j)
        if (lo + tid + 256 * j >= hi) xv[j] = -INFINITY;
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < kWideKeep; ++j)
        if (lo + tid + 256 * j < hi) mx = fmaxf(mx, xv[j]);
    mx = block_max(mx, red);
    float sum = 0.f;
    if (mx > -INFINITY) {
#pragma unroll
        for (int j = 0; j < kWideKeep; ++j)
            if (lo + tid + 256 * j < hi) sum += expf(xv[j] - mx);
    }
    sum = block_sum(sum, red);
    WidePartial* out = parts + (long)row * kSelBlocks + slice;
    if (tid == 0) { out->mx = mx; out->sum = sum; }
    // best entry of this thread strictly after (wv, wi) in the order (value descending, index ascending)
    auto best_after = [&](float wv, int wi, float& bv, int& bi) {
        bv = -INFINITY;
        bi = kWideNone;
#pragma unroll
        for (int j = 0; j < kWideKeep; ++j) {
            const int i = lo + tid + 256 * j;
            const float v = xv[j];
            const bool after = v < wv || (v == wv && i > wi);
            if (v > -INFINITY && after && (v > bv || (v == bv && i < bi))) { bv = v; bi = i; }
        }
    };
    float mv;
    int mi;
    best_after(INFINITY, -1, mv, mi);
    for (int round = 0; round < k; ++round) {
        float bv = mv;
        int bi = mi;
        wave_argmax(bv, bi);
        __syncthreads();                   // the previous round's fold has been read
        if ((tid & 63) == 0) { cand_v[tid >> 6] = bv; cand_i[tid >> 6] = bi; }
        __syncthreads();
        bv = cand_v[0];
        bi = cand_i[0];
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (cand_v[w] > bv || (cand_v[w] == bv && cand_i[w] < bi)) { bv = cand_v[w]; bi = cand_i[w]; }
        if (tid == 0) {
            out->v[round] = bv;
            out->i[round] = bi;
        }
        if (bi != kWideNone && mi == bi) best_after(bv, bi, mv, mi);
    }
}

__global__ __launch_bounds__(64) void topk_wide_stage2_kernel(const WidePartial* __restrict__ parts, int k,
                                                              float* __restrict__ top_vals, int* __restrict__ top_ids) {
    __shared__ float list_v[kWideTopK * 64];
    __shared__ int list_i[kWideTopK * 64];
    const int lane = threadIdx.x, row = blockIdx.x;
    const WidePartial* p = parts + (long)row * kSelBlocks + lane;
    const float pmx = p->mx, psum = p->sum;
#pragma unroll
    for (int t = 0; t < kWideTopK; ++t) {
        list_v[t * 64 + lane] = t < k ? p->v[t] : -INFINITY;
        list_i[t * 64 + lane] = t < k ? p->i[t] : kWideNone;
    }
    const float mx = wave_max(pmx);
    float sum = pmx > -INFINITY ? psum * expf(pmx - mx) : 0.f;
    sum = wave_sum(sum);
    const float lse = logf(sum);
    int head = 0;                          // next unconsumed entry of this slice's sorted list
    float cv = list_v[lane];
    int ci = list_i[lane];
    for (int round = 0; round < k; ++round) {
        float wv = cv;
        int wi = ci;
        wave_argmax(wv, wi);
        const bool some = wi != kWideNone;
        if (some && wi == ci) {
            ++head;
            const int h = head < kWideTopK ? head : kWideTopK - 1;
            cv = head < k ? list_v[h * 64 + lane] : -INFINITY;
            ci = head < k ? list_i[h * 64 + lane] : kWideNone;
        }
        if (lane == 0) {
            top_ids[row * k + round] = some ? wi : -1;
            top_vals[row * k + round] = some ? (wv - mx) - lse : -INFINITY;
        }
    }
}

void launch_logsoftmax_topk_wide(const LaunchCtx& ctx, const float* logits, int n_vocab, int n_rows, int k, float* top_vals,
                                 int* top_ids, void* scratch) {
    if (k < 1 || k > kWideTopK) throw std::invalid_argument("wide top-k: k must be in [1, 16]");
    if (n_rows < 1 || n_vocab < 1) throw std::invalid_argument("wide top-k: at least one row and one logit");
    if (!topk_wide_applicable(n_vocab, k))
        throw std::invalid_argument("wide top-k: rows of at most 262144 logits (a slice of 4096 held in registers)");
    WidePartial* parts = static_cast<WidePartial*>(scratch);
    {
        KernelScope ks(ctx, "sel_topk_wide_stage1", 0.0, 4.0 * n_rows * (double)n_vocab);
        hipLaunchKernelGGL(topk_wide_stage1_kernel, dim3(kSelBlocks, n_rows), dim3(256), 0, ctx.stream, logits, n_vocab, k,
                           parts);
        WLK_HIP(hipGetLastError());
    }
    {
        KernelScope ks(ctx, "sel_topk_wide_stage2");
        hipLaunchKernelGGL(topk_wide_stage2_kernel, dim3(n_rows), dim3(64), 0, ctx.stream, parts, k, top_vals, top_ids);
        WLK_HIP(hipGetLastError());
    }
}

size_t topk_wide_scratch_bytes(int n_rows) { return sizeof(WidePartial) * kSelBlocks * (size_t)n_rows; }

// softmax(logits)[token] of one row by one 1024-thread workgroup.  The row is read ONCE (each thread keeps its strided
// elements in registers between the max pass and the sum pass); the order of every max / sum is that of the plain
// two-pass loops.
__device__ __forceinline__ void token_prob_body(const float* __restrict__ logits, int n_vocab, int token,
                                                float* __restrict__ probs, int row) {
    __shared__ float red[16];
    constexpr int kKeep = 64;   // elements per thread held in registers: rows up to 65 536 logits
    const int tid = threadIdx.x;
    const float* x = logits + (long)row * n_vocab;
    float mx = -INFINITY, sum = 0.f;
    if (n_vocab <= kKeep * kSelThreads) {
        float v[kKeep];
#pragma unroll
        for (int j = 0; j < kKeep; ++j) {
            const int i = tid + j * kSelThreads;
            v[j] = i < n_vocab ? x[i] : -INFINITY;
        }
#pragma unroll
        for (int j = 0; j < kKeep; ++j) mx = fmaxf(mx, v[j]);
        mx = block_max(mx, red);
#pragma unroll
        for (int j = 0; j < kKeep; ++j)
            if (tid + j * kSelThreads < n_vocab) sum += expf(v[j] - mx);
    } else {
        for (int i = tid; i < n_vocab; i += kSelThreads) mx = fmaxf(mx, x[i]);
        mx = block_max(mx, red);
        for (int i = tid; i < n_vocab; i += kSelThreads) sum += expf(x[i] - mx);
    }
    sum = block_sum(sum, red);
    if (tid == 0) probs[row] = expf(x[token] - mx) / sum;
}

__global__ __launch_bounds__(kSelThreads) void token_prob_kernel(const float* __restrict__ logits, int n_vocab,
                                                                 int token, float* __restrict__ probs) {
    token_prob_body(logits, n_vocab, token, probs, blockIdx.x);
}

void launch_token_prob(const LaunchCtx& ctx, const float* logits, int n_vocab, int n_rows, int token, float* probs) {
    KernelScope ks(ctx, "sel_token_prob");
    hipLaunchKernelGGL(token_prob_kernel, dim3(n_rows), dim3(kSelThreads), 0, ctx.stream, logits, n_vocab, token,
                       probs);
    WLK_HIP(hipGetLastError());
}

// ---------------------------------------------------------------------------------------------
// AlignAtt.  Window rows of alignment head `a`, beam `b` live at ring[(a*n_beam+b)*ring_rows + r]:
// rows [0, prefill_rows) belong to the first step of this `infer` (as long as it is among the
// last 16 steps), rows single_base + [0, n_single) are later single-token steps.
// Step 1 (this kernel): per frame column, mean and population std over the window rows in fp64
// (torch.std_mean(unbiased=False) accumulates in double on CPU), then the z-score of the newest row.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void align_zscore_kernel(AlignArgs a) {
    align_zscore_body(a, blockIdx.x, blockIdx.y, blockIdx.z);
}

__device__ __forceinline__ float median7(float v0, float v1, float v2, float v3, float v4, float v5, float v6) {
    float v[7] = {v0, v1, v2, v3, v4, v5, v6};
#pragma unroll
    for (int i = 1; i < 7; ++i) {
#pragma unroll
        for (int j = i; j > 0; --j) {
            const float lo = fminf(v[j - 1], v[j]);
            const float hi = fmaxf(v[j - 1], v[j]);
            v[j - 1] = lo;
            v[j] = hi;
        }
    }
    return v[3];
}

// Step 2: one workgroup per beam row - median filter each head's z row (reflect padding over the
// full T before the content_mel_len cut, timing.py:35), average the heads, first arg-max.
__global__ __launch_bounds__(256) void align_argmax_kernel(AlignArgs a) {
    __shared__ float bestv[256];
    __shared__ int besti[256];
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    if (a.rows) a.content_len = a.rows[b].content_len;
    const float* zb = a.z + (long)b * a.n_align * a.T;
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int f = tid; f < a.T; f += 256) {
        float acc = 0.f;
        for (int al = 0; al < a.n_align; ++al) {
            const float* z = zb + (long)al * a.T;
            float v[7];
#pragma unroll
            for (int o = -3; o <= 3; ++o) {
                int idx = f + o;
                if (idx < 0) idx = -idx;
                if (idx >= a.T) idx = 2 * (a.T - 1) - idx;
                v[o + 3] = z[idx];
            }
            acc += a.T > 3 ? median7(v[0], v[1], v[2], v[3], v[4], v[5], v[6]) : z[f];
        }
        const float m = acc / (float)a.n_align;
        a.attn_last[(long)b * a.T + f] = m;
        if (f < a.content_len && (m > bv || (m == bv && f < bi))) { bv = m; bi = f; }
    }
    bestv[tid] = bv;
    besti[tid] = bi;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s) {
            const float ov = bestv[tid + s];
            const int oi = besti[tid + s];
            if (ov > bestv[tid] || (ov == bestv[tid] && oi < besti[tid])) { bestv[tid] = ov; besti[tid] = oi; }
        }
        __syncthreads();
    }
    if (tid == 0) a.frames[b] = besti[0] == 0x7fffffff ? 0 : besti[0];
}

// Step 2 variant for the common case (z of all alignment heads fits LDS): 1024 threads stage z with
// coalesced loads once, then medians / head mean / arg-max run out of LDS.
__device__ __forceinline__ void align_argmax_lds_body(AlignArgs a, int b, const StepHostOut host = StepHostOut{}, unsigned seq = 0) {
    extern __shared__ __attribute__((aligned(16))) float zs[];   // [n_align][T]
    __shared__ float bestv[16];
    __shared__ int besti[16];
    const int tid = threadIdx.x;
    if (a.rows) a.content_len = a.rows[b].content_len;
    const float* zb = a.z + (long)b * a.n_align * a.T;
    for (int i = tid; i < a.n_align * a.T; i += 1024) zs[i] = zb[i];
    asm volatile("" : "+v"(seq));   // requested with the z rows, not in front of the flag store at the very end
    __syncthreads();
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int f = tid; f < a.T; f += 1024) {
        float acc = 0.f;
        for (int al = 0; al < a.n_align; ++al) {
            const float* z = zs + al * a.T;
            float v[7];
#pragma unroll
            for (int o = -3; o <= 3; ++o) {
                int idx = f + o;
                if (idx < 0) idx = -idx;
                if (idx >= a.T) idx = 2 * (a.T - 1) - idx;
                v[o + 3] = z[idx];
            }
            acc += a.T > 3 ? median7(v[0], v[1], v[2], v[3], v[4], v[5], v[6]) : z[f];
        }
        const float m = acc / (float)a.n_align;
        a.attn_last[(long)b * a.T + f] = m;
        if (f < a.content_len && (m > bv || (m == bv && f < bi))) { bv = m; bi = f; }
    }
    // (value, frame) arg-max with ties to the lowest frame: order-free, so sixteen VALU butterflies + one 16-entry fold
    // replace the ten-level LDS tree and its ten barriers
    wave_argmax(bv, bi);
    if ((tid & 63) == 0) { bestv[tid >> 6] = bv; besti[tid >> 6] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 16; ++w)
            if (bestv[w] > bestv[0] || (bestv[w] == bestv[0] && besti[w] < besti[0])) { bestv[0] = bestv[w]; besti[0] = besti[w]; }
    }
    if (tid == 0) {
        const int frame = besti[0] == 0x7fffffff ? 0 : besti[0];
        a.frames[b] = frame;
        if (host.result) {
            host.result[b].frame = frame;
            publish_flag(&host.result[b].flag_align, seq);
        }
    }
}

__global__ __launch_bounds__(1024) void align_argmax_lds_kernel(AlignArgs a) { align_argmax_lds_body(a, blockIdx.x); }

// ---------------------------------------------------------------------------------------------
// The tail of a decode step in TWO launches instead of four: the slice pass of the top-k and the z-score of the
// alignment window are independent (logits vs cross-attention rows), and so are their second stages; each pair shares a
// launch, workgroups pick their role from the block index.  Same device functions, same arithmetic as the four
// separate kernels above (which remain for the configurations the fused form does not cover).
// ---------------------------------------------------------------------------------------------
// every field either role reads, requested by one s_load burst at kernel entry (see WLK_PIN_GEMM_ARGS)
#define WLK_PIN_SELECT_ARGS(t, a)                                                                                           \
    do {                                                                                                                    \
        asm volatile("" ::"s"((t).logits), "s"((t).n_vocab), "s"((t).k), "s"((t).n_rows), "s"((t).parts), "s"((t).adj_row), \
                     "s"((t).adj_ids), "s"((t).adj_deltas), "s"((t).n_adj), "s"((t).top_vals), "s"((t).top_ids),            \
                     "s"((t).host.result), "s"((t).host.n_adj), "s"((t).host.seq));                                         \
        asm volatile("" ::"s"((a).ring), "s"((a).n_align), "s"((a).n_beam), "s"((a).ring_rows), "s"((a).T),                 \
                     "s"((a).prefill_rows), "s"((a).n_single), "s"((a).newest_row), "s"((a).single_base),                   \
                     "s"((a).content_len), "s"((a).z), "s"((a).attn_last), "s"((a).frames), "s"((a).rows));                 \
        __builtin_amdgcn_sched_barrier(0);                                                                                  \
    } while (0)

__global__ __launch_bounds__(256) void select_stage1_kernel(TopkArgs t, AlignArgs a, int zf_blocks) {
    WLK_PIN_SELECT_ARGS(t, a);
    const int n_topk = kSelBlocks * t.n_rows;
    if ((int)blockIdx.x < n_topk) {
        const int n_adj = t.host.n_adj ? *t.host.n_adj : t.n_adj;
        topk_stage1_body(t.logits, t.n_vocab, t.k, t.parts, t.adj_row, t.adj_ids, t.adj_deltas, n_adj,
                         blockIdx.x % kSelBlocks, blockIdx.x / kSelBlocks);
    } else {
        const int i = blockIdx.x - n_topk;
        const int fblock = i % zf_blocks, rest = i / zf_blocks;
        align_zscore_body(a, fblock, rest % a.n_align, rest / a.n_align);
    }
}

__global__ __launch_bounds__(1024) void select_stage2_kernel(TopkArgs t, AlignArgs a) {
    WLK_PIN_SELECT_ARGS(t, a);
    // the step's sequence number (echoed in the result flags) is requested here, not in front of the flag store at the
    // very end of the step's last kernel - the host is waiting on exactly that store
    unsigned seq = 0;
    if (t.host.result) seq = *t.host.seq;     // (each role pins it behind its first batch of loads: one round trip with them)
    if ((int)blockIdx.x < a.n_beam) {
        align_argmax_lds_body(a, blockIdx.x, t.host, seq);
    } else if ((int)blockIdx.x < a.n_beam + t.n_rows) {
        if (threadIdx.x < 64) topk_stage2_body(t.parts, t.k, t.top_vals, t.top_ids, blockIdx.x - a.n_beam, t.host, seq);
    } else {
        token_prob_body(t.ns_logits, t.n_vocab, t.ns_token, t.ns_probs, blockIdx.x - a.n_beam - t.n_rows);
    }
}

// Graph-replayed single-session steps (round 6, `early_z`).  The z-score has already run beside the vocabulary projection
// (gemv_f32_kernel's side workgroups).  What the trace of the first form of this showed: the medians are VALU work - 1 500
// frames x 5 heads x 21 compare-exchanges - and ONE workgroup (one compute unit) needs 9-11 us for them however it is
// scheduled.  So the medians / head mean run as (T + 255) / 256 workgroups of the top-k SLICE pass's launch, one frame per
// thread, each leaving the (value, lowest frame) arg-max of its 256 frames; the step's last launch is one wave that folds the
// 64 slices of the top-k and the frame blocks of the read-out, stores both into the host's result block and raises both
// flags behind one system-scope fence.  Same per-frame expressions as align_argmax_lds_body, and an arg-max with ties to the
// lowest frame does not depend on how it is grouped: the step's numbers are those of the two launches above.
constexpr int kAlignPartFrames = 256;
__device__ __forceinline__ void align_median_part_body(AlignArgs a, int b, int blk, int n_blk) {
    __shared__ float bestv[4];
    __shared__ int besti[4];
    const int tid = threadIdx.x;
    if (a.rows) a.content_len = a.rows[b].content_len;
    const float* zb = a.z + (long)b * a.n_align * a.T;
    const int f = blk * kAlignPartFrames + tid;
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    if (f < a.T) {
        float acc = 0.f;
        for (int al = 0; al < a.n_align; ++al) {
            const float* z = zb + (long)al * a.T;
            float v[7];
#pragma unroll
            for (int o = -3; o <= 3; ++o) {
                int idx = f + o;
                if (idx < 0) idx = -idx;
                if (idx >= a.T) idx = 2 * (a.T - 1) - idx;
                v[o + 3] = z[idx];
            }
            acc += a.T > 3 ? median7(v[0], v[1], v[2], v[3], v[4], v[5], v[6]) : z[f];
        }
        const float m = acc / (float)a.n_align;
        a.attn_last[(long)b * a.T + f] = m;
        if (f < a.content_len && (m > bv || (m == bv && f < bi))) { bv = m; bi = f; }
    }
    wave_argmax(bv, bi);
    if ((tid & 63) == 0) { bestv[tid >> 6] = bv; besti[tid >> 6] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w)
            if (bestv[w] > bestv[0] || (bestv[w] == bestv[0] && besti[w] < besti[0])) { bestv[0] = bestv[w]; besti[0] = besti[w]; }
        float* slot = a.part + ((long)b * 64 + blk) * 2;
        slot[0] = bestv[0];
        slot[1] = __int_as_float(besti[0]);
    }
}

__global__ __launch_bounds__(256) void select_stage1_early_kernel(TopkArgs t, AlignArgs a, int n_blk) {
    WLK_PIN_SELECT_ARGS(t, a);
    const int n_topk = kSelBlocks * t.n_rows;
    if ((int)blockIdx.x < n_topk) {
        const int n_adj = t.host.n_adj ? *t.host.n_adj : t.n_adj;
        topk_stage1_body(t.logits, t.n_vocab, t.k, t.parts, t.adj_row, t.adj_ids, t.adj_deltas, n_adj,
                         blockIdx.x % kSelBlocks, blockIdx.x / kSelBlocks);
    } else {
        const int i = blockIdx.x - n_topk;
        align_median_part_body(a, i / n_blk, i % n_blk, n_blk);
    }
}

// one wave per row: lane = top-k slice, and lane = frame block of the read-out (n_blk <= 64)
__global__ __launch_bounds__(64) void select_stage2_early_kernel(TopkArgs t, AlignArgs a, int n_blk) {
    asm volatile("" ::"s"(t.parts), "s"(t.k), "s"(t.top_vals), "s"(t.top_ids), "s"(t.host.result), "s"(t.host.seq), "s"(a.part),
                 "s"(a.frames));
    __builtin_amdgcn_sched_barrier(0);
    const int row = blockIdx.x, lane = threadIdx.x;
    unsigned seq = 0;
    if (t.host.result) seq = *t.host.seq;
    const float* slot = a.part + ((long)row * 64 + (lane < n_blk ? lane : 0)) * 2;
    float bv = slot[0];
    int bi = __float_as_int(slot[1]);
    if (lane >= n_blk) { bv = -INFINITY; bi = 0x7fffffff; }
    topk_stage2_body(t.parts, t.k, t.top_vals, t.top_ids, row, t.host, seq, false);
    // a block whose frames all lie behind content_len (or are NaN) left (-inf, 0x7fffffff): it loses every comparison, as
    // its threads' candidates do in the one-workgroup form
    wave_argmax(bv, bi);
    if (lane == 0) {
        const int frame = bi == 0x7fffffff ? 0 : bi;
        a.frames[row] = frame;
        if (t.host.result) {
            t.host.result[row].frame = frame;
            __threadfence_system();
            __hip_atomic_store(&t.host.result[row].flag_topk, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(&t.host.result[row].flag_align, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

bool select_early_z_enabled() {
    // read per call (a session asks once, when it captures its step graph): tests flip WLK_EARLY_Z inside one process
    const char* e = getenv("WLK_EARLY_Z");
    return !(e && e[0] == '0');
}

bool select_fused_applicable(int n_rows, int k, const AlignArgs& a) {
    static const bool enabled = [] {
        const char* e = getenv("WLK_SELECT_FUSED");
        return !(e && e[0] == '0');
    }();
    const size_t lds = (size_t)a.n_align * a.T * sizeof(float);
    return enabled && a.n_align > 0 && a.n_beam == n_rows && lds + 8192 + 1024 <= 150 * 1024 && k >= 1 && k <= kMaxTopK;
}

bool launch_select_fused(const LaunchCtx& ctx, float* logits, int n_vocab, int n_rows, int k, float* top_vals, int* top_ids,
                         void* scratch, const int* adj_row, const int* adj_ids, const float* adj_deltas, int n_adj,
                         const AlignArgs& a, const StepHostOut& host, const float* ns_logits, int ns_token, float* ns_probs,
                         bool early_z) {
    const size_t lds = (size_t)a.n_align * a.T * sizeof(float);
    if (!select_fused_applicable(n_rows, k, a)) return false;
    static std::atomic<bool> attr_set[64];
    int dev = 0;
    WLK_HIP(hipGetDevice(&dev));
    if (dev < 64 && !attr_set[dev].load(std::memory_order_acquire)) {
        WLK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(select_stage2_kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
        attr_set[dev].store(true, std::memory_order_release);
    }
    TopkArgs t{logits, n_vocab, k, n_rows, static_cast<SelPartial*>(scratch), adj_row, adj_ids, adj_deltas, n_adj, top_vals, top_ids,
               host, ns_logits, ns_token, ns_probs};
    const int zf = (a.T + 63) / 64;
    if (early_z) {
        const int n_blk = (a.T + kAlignPartFrames - 1) / kAlignPartFrames;
        if (ns_logits || !a.part || n_blk > 64) throw std::invalid_argument("select: the early z-score form needs a.part, T <= 16384 and no no-speech block");
        {
            KernelScope ks(ctx, "sel_stage1", 0.0, 4.0 * 3.0 * n_rows * (double)n_vocab);
            hipLaunchKernelGGL(select_stage1_early_kernel, dim3(kSelBlocks * n_rows + n_blk * a.n_beam), dim3(256), 0, ctx.stream, t, a, n_blk);
            WLK_HIP(hipGetLastError());
        }
        {
            KernelScope ks(ctx, "sel_stage2");
            hipLaunchKernelGGL(select_stage2_early_kernel, dim3(n_rows), dim3(64), 0, ctx.stream, t, a, n_blk);
            WLK_HIP(hipGetLastError());
        }
        return true;
    }
    {
        KernelScope ks(ctx, "sel_stage1", 0.0, 4.0 * 3.0 * n_rows * (double)n_vocab);
        hipLaunchKernelGGL(select_stage1_kernel, dim3(kSelBlocks * n_rows + zf * a.n_align * a.n_beam), dim3(256), 0,
                           ctx.stream, t, a, zf);
        WLK_HIP(hipGetLastError());
    }
    {
        KernelScope ks(ctx, "sel_stage2");
        hipLaunchKernelGGL(select_stage2_kernel, dim3(a.n_beam + n_rows + (ns_logits ? n_rows : 0)), dim3(1024), lds,
                           ctx.stream, t, a);
        WLK_HIP(hipGetLastError());
    }
    return true;
}

// ---------------------------------------------------------------------------------------------
// The per-step logit rules of whisper's batch decoder (whisper/decoding.py:417-499: SuppressBlank, SuppressTokens,
// ApplyTimestampRules) and the greedy pick at temperature 0 (GreedyDecoder.update, :270-287) for ONE sequence, on the device:
// the host keeps what the rules need of the token history (three flags and a bound) and reads back the token and its
// log-probability - 8 bytes per step instead of the 207 KB logits row, and no 52k-element log_softmax on the host.
//   allowed(v) = not suppressed, not a blank at the first step, and (with timestamps) none of: <|notimestamps|>; a timestamp
//   behind a closed pair (mode 1); a text token behind an opening timestamp (mode 2); a timestamp below the monotonic bound;
//   at the first step a text token or a timestamp beyond max_initial.
//   Then, as the reference: if logsumexp(logprobs[timestamps]) > max(logprobs[text]) the text tokens go too.
//   token = argmax over what is left (lowest index on ties), log-probability = log_softmax over what is left at that
//   token = -log(sum exp(x - max)).
// One workgroup of 1024 threads, two strided passes over the row (51 elements per thread).
// ---------------------------------------------------------------------------------------------
namespace {
struct PickBest {
    float v;
    int i;
};
__device__ __forceinline__ PickBest pick_better(PickBest a, PickBest b) {      // larger value, lower index on ties
    return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a;
}
__device__ __forceinline__ PickBest pick_wave_best(PickBest x) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        PickBest o;
        o.v = __shfl_xor(x.v, off);
        o.i = __shfl_xor(x.i, off);
        x = pick_better(x, o);
    }
    return x;
}
// allowed(v) of the header comment: one statement of the rules for the one-row pick and the n-row top-k
__device__ __forceinline__ bool rules_allowed(const unsigned char* __restrict__ mask, const PickRules& p, int v) {
    const int tb = p.timestamp_begin;
    const unsigned char m = mask[v];
    if ((m & 1) || (p.first_step && (m & 2))) return false;
    if (p.without_timestamps) return true;
    if (v == p.no_timestamps) return false;
    if (p.ts_mode == 1 && v >= tb) return false;
    if (p.ts_mode == 2 && v < p.eot) return false;
    if (v >= tb && v < p.ts_bound) return false;
    if (p.first_step && (v < tb || (p.max_initial >= 0 && v >= tb + p.max_initial + 1))) return false;
    return true;
}
}  // namespace

// The pick of one row by one 1024-thread workgroup: the one statement of it for wlk_pick_greedy's single row
// (rules_pick_kernel) and for the rows of a window group (rules_pick_rows_kernel).  Thread t owns entries t, t + 1024, ... in
// ascending order and every reduction folds in a fixed order, so the two kernels give the same bits for the same row.
//   kRegs = false: two strided passes over memory (51 elements per thread).
//   kRegs = true (rows of at most kRulesKeep * 1024 entries: every Whisper vocabulary): the row is read ONCE, all of a
//     thread's loads issued ahead of the first reduction, an entry the rules forbid remembered in a 64-bit set.  The loads
//     stay one dword per lane (a wave reads 256 contiguous bytes): a 16-byte load per lane would hand a thread four
//     NEIGHBOURING entries, i.e. another summation order than the one-row kernel's, and its bits are the contract.
constexpr int kRulesKeep = 52;
template <bool kRegs>
__device__ __forceinline__ void rules_pick_body(const float* __restrict__ logits, int n_vocab,
                                                const unsigned char* __restrict__ mask, const PickRules& p,
                                                int* __restrict__ out_token, float* __restrict__ out_logprob) {
    __shared__ PickBest s_all[16], s_ts[16];
    __shared__ float s_text[16], s_sum_all[16], s_sum_ts[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tb = p.timestamp_begin;
    float xv[kRegs ? kRulesKeep : 1];
    unsigned long long ok = 0ull;
    if constexpr (kRegs) {
#pragma unroll
        for (int j = 0; j < kRulesKeep; ++j) {
            const int v = tid + 1024 * j, vc = v < n_vocab ? v : 0;
            xv[j] = logits[vc];
            if (v < n_vocab && rules_allowed(mask, p, vc)) ok |= 1ull << j;
        }
    }
    // f(index, logit) over this thread's allowed entries, ascending index
    auto sweep = [&](auto&& f) {
        if constexpr (kRegs) {
#pragma unroll
            for (int j = 0; j < kRulesKeep; ++j)
                if ((ok >> j) & 1ull) f(tid + 1024 * j, xv[j]);
        } else {
            for (int v = tid; v < n_vocab; v += 1024)
                if (rules_allowed(mask, p, v)) f(v, logits[v]);
        }
    };
    PickBest all{-INFINITY, 0x7fffffff}, ts{-INFINITY, 0x7fffffff};
    float text = -INFINITY;
    sweep([&](int v, float x) {
        all = pick_better(all, PickBest{x, v});
        if (v >= tb) ts = pick_better(ts, PickBest{x, v});
        else text = fmaxf(text, x);
    });
    all = pick_wave_best(all);
    ts = pick_wave_best(ts);
    text = wave_max(text);
    if (lane == 0) {
        s_all[wave] = all;
        s_ts[wave] = ts;
        s_text[wave] = text;
    }
    __syncthreads();
    all = s_all[0];
    ts = s_ts[0];
    text = s_text[0];
#pragma unroll
    for (int w = 1; w < 16; ++w) {
        all = pick_better(all, s_all[w]);
        ts = pick_better(ts, s_ts[w]);
        text = fmaxf(text, s_text[w]);
    }
    float sum_all = 0.f, sum_ts = 0.f;
    sweep([&](int v, float x) {
        sum_all += expf(x - all.v);
        if (v >= tb) sum_ts += expf(x - ts.v);
    });
    sum_all = wave_sum(sum_all);
    sum_ts = wave_sum(sum_ts);
    if (lane == 0) {
        s_sum_all[wave] = sum_all;
        s_sum_ts[wave] = sum_ts;
    }
    __syncthreads();
    if (tid == 0) {
        sum_all = 0.f;
        sum_ts = 0.f;
        for (int w = 0; w < 16; ++w) {
            sum_all += s_sum_all[w];
            sum_ts += s_sum_ts[w];
        }
        const float lse_all = all.v + logf(sum_all);
        // logsumexp(logprobs[tb:]) > logprobs[:tb].max(), both relative to the same log_softmax
        const bool ts_wins = !p.without_timestamps && ts.i != 0x7fffffff && (ts.v + logf(sum_ts)) - lse_all > text - lse_all;
        const PickBest pick = ts_wins ? ts : all;
        out_token[0] = pick.i == 0x7fffffff ? 0 : pick.i;
        out_logprob[0] = -logf(ts_wins ? sum_ts : sum_all);
    }
}

__global__ __launch_bounds__(1024) void rules_pick_kernel(const float* __restrict__ logits, int n_vocab,
                                                          const unsigned char* __restrict__ mask, PickRules p,
                                                          int* __restrict__ out_token, float* __restrict__ out_logprob) {
    rules_pick_body<false>(logits, n_vocab, mask, p, out_token, out_logprob);
}

// The same pick for the rows of a window group (window_group.hip): one workgroup per row, all rows in flight side by side.
// Row r reads logits row r, its own rules and its own mask (two sessions may carry different wlk_rules_set lists) from the
// device table and writes (token, log-probability) to slot r of `out` - one 8 n byte read-back for the host.
__global__ __launch_bounds__(1024) void rules_pick_rows_kernel(const float* __restrict__ logits, int n_vocab,
                                                               const PickRowEntry* __restrict__ table, int* __restrict__ out) {
    const int row = blockIdx.x;
    const PickRowEntry e = table[row];
    const float* x = logits + (long)row * n_vocab;
    int* o = out + 2 * row;
    if (n_vocab <= kRulesKeep * 1024) rules_pick_body<true>(x, n_vocab, e.mask, e.p, o, reinterpret_cast<float*>(o + 1));
    else rules_pick_body<false>(x, n_vocab, e.mask, e.p, o, reinterpret_cast<float*>(o + 1));
}

void launch_rules_pick_rows(const LaunchCtx& ctx, const float* logits, int n_vocab, int n_rows, const PickRowEntry* table, int* out) {
    if (n_rows < 1 || n_rows > kMaxPickRows) throw std::invalid_argument("rules pick: 1..8 rows");
    KernelScope ks(ctx, "rules_pick_rows", 0.0, 5.0 * n_rows * (double)n_vocab);
    hipLaunchKernelGGL(rules_pick_rows_kernel, dim3(n_rows), dim3(1024), 0, ctx.stream, logits, n_vocab, table, out);
    WLK_HIP(hipGetLastError());
}

// Draft verification (window_group.hip: wlk_group_verify): the greedy pick at EVERY candidate position of a
// teacher-forced window in one launch.  Workgroup j = the position behind draft[0 .. j): logits row j, the session's mask,
// and the rule state that position has - the window's first-pick state walked through pick_rules_advance over draft[0 .. j)
// by one lane (at most 255 steps of a dozen integer operations; the one statement of the transition stays common.h's).
// The pick itself is rules_pick_body in the form rules_pick_rows_kernel takes (same loads, same fold order), so a
// position's (token, log-probability) are the bits wlk_pick_greedy gives on that row, mask and state.
//   out[3 j] = token, out[3 j + 1] = log-probability bits, out[3 j + 2] = j < n_draft && token == draft[j]
__global__ __launch_bounds__(1024) void draft_pick_rows_kernel(const float* __restrict__ logits, int n_vocab,
                                                               const unsigned char* __restrict__ mask, PickRules p0,
                                                               const int* __restrict__ draft, int n_draft,
                                                               int* __restrict__ out) {
    __shared__ PickRules s_rules;
    __shared__ int s_token;
    __shared__ float s_logprob;
    const int j = blockIdx.x;
    if (threadIdx.x == 0) {
        PickRules q = p0;
        for (int i = 0; i < j && i < n_draft; ++i) q = pick_rules_advance(q, draft[i]);
        s_rules = q;
    }
    __syncthreads();
    const PickRules p = s_rules;
    const float* x = logits + (long)j * n_vocab;
    if (n_vocab <= kRulesKeep * 1024) rules_pick_body<true>(x, n_vocab, mask, p, &s_token, &s_logprob);
    else rules_pick_body<false>(x, n_vocab, mask, p, &s_token, &s_logprob);
    __syncthreads();
    if (threadIdx.x == 0) {
        const int token = s_token;
        out[3 * j] = token;
        out[3 * j + 1] = __float_as_int(s_logprob);
        out[3 * j + 2] = (j < n_draft && token == draft[j]) ? 1 : 0;
    }
}

// One wave per window behind draft_pick_rows_kernel: k = the first position whose pick is not the draft's token (a ballot
// over the match flags, 64 positions a round; n_draft when every one matches), next = the pick at k, and the sum of the
// log-probabilities of positions 0 .. k, added in ascending order by one lane, one fp32 add after the other - the order
// in which transcribe._greedy_take accumulates, so the sum has the host loop's bits for the same addends.  `ended`: the
// token in front of position 0 was <|endoftext|> already; _greedy_take then takes <|endoftext|> whatever was picked and
// adds nothing (a draft token never is <|endoftext|>, so no later position can be in that state).
//   res[0] = k, res[1] = next token, res[2] = its log-probability bits, res[3] = the sum's bits
__global__ __launch_bounds__(64) void draft_accept_kernel(const int* __restrict__ picks, int n_draft, int eot, int ended,
                                                          int* __restrict__ res) {
    const int lane = threadIdx.x;
    int k = n_draft;
    for (int base = 0; base < n_draft; base += 64) {
        const int j = base + lane;
        const bool miss = j < n_draft && (picks[3 * j + 2] == 0 || (ended && j == 0));
        const unsigned long long m = __ballot(miss);
        if (m != 0ull) {
            k = base + __ffsll((long long)m) - 1;
            break;
        }
    }
    if (lane == 0) {
        float sum = 0.f;
        for (int j = ended ? 1 : 0; j <= k; ++j) sum += __int_as_float(picks[3 * j + 1]);
        res[0] = k;
        res[1] = (ended && k == 0) ? eot : picks[3 * k];
        res[2] = picks[3 * k + 1];
        res[3] = __float_as_int(sum);
    }
}

// the logits row wlk_group_verify leaves in the session: row res[0] (the accepted count, known on the device only while the
// logits buffer is reused by the next window) of `logits` to `dst`, a plain copy
__global__ __launch_bounds__(256) void draft_keep_row_kernel(const float* __restrict__ logits, int n_vocab,
                                                             const int* __restrict__ res, int n_rows, float* __restrict__ dst) {
    const int k = res[0];
    if (k < 0 || k >= n_rows) return;
    const float* src = logits + (long)k * n_vocab;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n_vocab; i += gridDim.x * 256) dst[i] = src[i];
}

void launch_draft_pick(const LaunchCtx& ctx, const float* logits, int n_vocab, const unsigned char* mask, const PickRules& p0,
                       const int* draft, int n_draft, int ended, int* picks, int* res, float* keep_row) {
    if (n_draft < 1 || n_draft > kMaxDraft) throw std::invalid_argument("draft pick: 1..256 draft tokens");
    {
        KernelScope ks(ctx, "draft_pick_rows", 0.0, 5.0 * (n_draft + 1) * (double)n_vocab);
        hipLaunchKernelGGL(draft_pick_rows_kernel, dim3(n_draft + 1), dim3(1024), 0, ctx.stream, logits, n_vocab, mask, p0, draft,
                           n_draft, picks);
        WLK_HIP(hipGetLastError());
    }
    {
        KernelScope ks(ctx, "draft_accept");
        hipLaunchKernelGGL(draft_accept_kernel, dim3(1), dim3(64), 0, ctx.stream, picks, n_draft, p0.eot, ended, res);
        WLK_HIP(hipGetLastError());
    }
    if (keep_row) {
        KernelScope ks(ctx, "draft_keep_row", 0.0, 8.0 * n_vocab);
        hipLaunchKernelGGL(draft_keep_row_kernel, dim3(32), dim3(256), 0, ctx.stream, logits, n_vocab, res, n_draft + 1, keep_row);
        WLK_HIP(hipGetLastError());
    }
}

void launch_rules_pick(const LaunchCtx& ctx, const float* logits, int n_vocab, const unsigned char* mask, const PickRules& p,
                       int* out_token, float* out_logprob) {
    KernelScope ks(ctx, "rules_pick", 0.0, 8.0 * n_vocab);
    hipLaunchKernelGGL(rules_pick_kernel, dim3(1), dim3(1024), 0, ctx.stream, logits, n_vocab, mask, p, out_token, out_logprob);
    WLK_HIP(hipGetLastError());
}

// ---------------------------------------------------------------------------------------------
// The same rules for the B rows of a beam session (batch `transcribe` with beam_size 2..7), each row with its own timestamp
// history, and the k best log-probabilities of every row instead of the arg-max: what BeamSearchDecoder.update
// (decoding.py:332-338) reads, k = beam + 1.  One 1024-thread workgroup per row.
//   * The row is read ONCE: thread t keeps entries t, t + 1024, ... in registers (kRulesKeep = 52 of them: every Whisper
//     vocabulary), an entry the rules forbid as -inf.  Longer rows (kRegs = false) re-read memory in every sweep instead.
//   * max and sum exp(x - max) over the allowed set and over the allowed timestamps, the "timestamps outweigh text"
//     decision in the host's form (logsumexp(logprobs[tb:]) > max(logprobs[:tb]), both under the same log_softmax); when the
//     timestamps win the text entries drop out and the normaliser is the timestamps' sum.
//   * the k best by (value descending, index ascending) in k rounds of exclusion: every thread holds the best entry it has
//     left, a round is one wave_argmax butterfly + a 16-entry fold through LDS, and only the thread that owned the winner
//     looks for its next entry ("after the winner" in that order - which also excludes everything it gave up before).
//     Chosen over per-thread sorted lists + merge: a list of k per thread is k * 2 more registers and a runtime-indexed
//     head, for rounds that here cost one 52-entry register scan in one thread.
//   logprob = (x - max) - logf(sum); a row with fewer than k allowed (finite) entries fills up with (-inf, -1).
// ---------------------------------------------------------------------------------------------
namespace {
// x comes strictly after w in the order (value descending, index ascending)
__device__ __forceinline__ bool pick_after(float xv, int xi, PickBest w) { return xv < w.v || (xv == w.v && xi > w.i); }
}  // namespace

template <bool kRegs>
__device__ __forceinline__ void rules_topk_body(const float* __restrict__ x, int n_vocab, const unsigned char* __restrict__ mask,
                                                const PickRules& p, int k, float* __restrict__ out_lp,
                                                int* __restrict__ out_ids) {
    __shared__ PickBest s_best[16];
    __shared__ float s_a[16], s_b[16], s_c[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tb = p.timestamp_begin;
    float xv[kRegs ? kRulesKeep : 1];
    if constexpr (kRegs) {
#pragma unroll
        for (int j = 0; j < kRulesKeep; ++j) {
            const int v = tid + 1024 * j, vc = v < n_vocab ? v : 0;
            const float raw = x[vc];
            xv[j] = (v < n_vocab && rules_allowed(mask, p, vc)) ? raw : -INFINITY;
        }
    }
    // f(index, value under the rules) over this thread's entries, ascending index
    auto sweep = [&](auto&& f) {
        if constexpr (kRegs) {
#pragma unroll
            for (int j = 0; j < kRulesKeep; ++j) f(tid + 1024 * j, xv[j]);
        } else {
            for (int v = tid; v < n_vocab; v += 1024) f(v, rules_allowed(mask, p, v) ? x[v] : -INFINITY);
        }
    };
    float m_ts = -INFINITY, m_text = -INFINITY;
    sweep([&](int v, float val) {
        if (v >= tb) m_ts = fmaxf(m_ts, val);
        else m_text = fmaxf(m_text, val);
    });
    m_ts = wave_max(m_ts);
    m_text = wave_max(m_text);
    if (lane == 0) {
        s_a[wave] = m_ts;
        s_b[wave] = m_text;
    }
    __syncthreads();
    m_ts = s_a[0];
    m_text = s_b[0];
#pragma unroll
    for (int w = 1; w < 16; ++w) {
        m_ts = fmaxf(m_ts, s_a[w]);
        m_text = fmaxf(m_text, s_b[w]);
    }
    const float m_all = fmaxf(m_ts, m_text);
    float sum_all = 0.f, sum_ts = 0.f;
    sweep([&](int v, float val) {
        if (val > -INFINITY) {
            sum_all += expf(val - m_all);
            if (v >= tb) sum_ts += expf(val - m_ts);
        }
    });
    sum_all = wave_sum(sum_all);
    sum_ts = wave_sum(sum_ts);
    __syncthreads();                       // the maxima have been read
    if (lane == 0) {
        s_a[wave] = sum_all;
        s_c[wave] = sum_ts;
    }
    __syncthreads();
    sum_all = 0.f;
    sum_ts = 0.f;
#pragma unroll
    for (int w = 0; w < 16; ++w) {        // every thread folds the 16 partials in the same order
        sum_all += s_a[w];
        sum_ts += s_c[w];
    }
    const float lse_all = m_all + logf(sum_all);
    const bool ts_wins = !p.without_timestamps && m_ts > -INFINITY && (m_ts + logf(sum_ts)) - lse_all > m_text - lse_all;
    const float mx = ts_wins ? m_ts : m_all;
    const float logsum = logf(ts_wins ? sum_ts : sum_all);
    const int lo = ts_wins ? tb : 0;       // timestamps as a group outweigh every text token: the text entries drop out

    auto best_after = [&](PickBest w) {
        PickBest b{-INFINITY, 0x7fffffff};
        sweep([&](int v, float val) {
            if (v >= lo && val > -INFINITY && pick_after(val, v, w)) b = pick_better(b, PickBest{val, v});
        });
        return b;
    };
    PickBest mine = best_after(PickBest{INFINITY, -1});
    for (int round = 0; round < k; ++round) {
        PickBest w = mine;
        wave_argmax(w.v, w.i);
        __syncthreads();                   // the previous round's fold has been read
        if (lane == 0) s_best[wave] = w;
        __syncthreads();
        w = s_best[0];
#pragma unroll
        for (int i = 1; i < 16; ++i) w = pick_better(w, s_best[i]);
        const bool some = w.i != 0x7fffffff;
        if (tid == 0) {
            out_ids[round] = some ? w.i : -1;
            out_lp[round] = some ? (w.v - mx) - logsum : -INFINITY;
        }
        if (some && mine.i == w.i) mine = best_after(w);
    }
}

__global__ __launch_bounds__(1024) void rules_topk_kernel(const float* __restrict__ logits, int n_vocab,
                                                          const unsigned char* __restrict__ mask, PickRulesRows rules, int k,
                                                          float* __restrict__ out_lp, int* __restrict__ out_ids) {
    const int row = blockIdx.x;
    const PickRules p = rules.r[row];
    const float* x = logits + (long)row * n_vocab;
    if (n_vocab <= kRulesKeep * 1024) rules_topk_body<true>(x, n_vocab, mask, p, k, out_lp + row * k, out_ids + row * k);
    else rules_topk_body<false>(x, n_vocab, mask, p, k, out_lp + row * k, out_ids + row * k);
}

void launch_rules_topk(const LaunchCtx& ctx, const float* logits, int n_vocab, int n_rows, const unsigned char* mask,
                       const PickRulesRows& rules, int k, float* out_lp, int* out_ids) {
    if (n_rows < 1 || n_rows > kMaxPickRows || k < 1 || k > kMaxTopK) throw std::invalid_argument("rules top-k: 1..8 rows, k in [1, 8]");
    KernelScope ks(ctx, "rules_topk", 0.0, 5.0 * n_rows * (double)n_vocab);
    hipLaunchKernelGGL(rules_topk_kernel, dim3(n_rows), dim3(1024), 0, ctx.stream, logits, n_vocab, mask, rules, k, out_lp,
                       out_ids);
    WLK_HIP(hipGetLastError());
}

void launch_alignatt_rows(const LaunchCtx& ctx, const AlignArgs& a0, const StepRow* rows) {
    AlignArgs a = a0;
    a.rows = rows;
    launch_alignatt(ctx, a);
}

void launch_align_zscore(const LaunchCtx& ctx, const AlignArgs& a) {
    const int n = a.rows ? kAlignWindow : a.prefill_rows + a.n_single;
    KernelScope ks(ctx, "align_zscore", 0.0, 4.0 * 2.0 * n * (double)a.n_align * a.T * a.n_beam);
    hipLaunchKernelGGL(align_zscore_kernel, dim3((a.T + 63) / 64, a.n_align, a.n_beam), dim3(256), 0, ctx.stream, a);
    WLK_HIP(hipGetLastError());
}

void launch_align_argmax_plain(const LaunchCtx& ctx, const AlignArgs& a) {
    KernelScope ks(ctx, "align_argmax");
    hipLaunchKernelGGL(align_argmax_kernel, dim3(a.n_beam), dim3(256), 0, ctx.stream, a);
    WLK_HIP(hipGetLastError());
}

void launch_alignatt(const LaunchCtx& ctx, const AlignArgs& a) {
    if (a.n_align <= 0) {
        WLK_HIP(hipMemsetAsync(a.frames, 0, sizeof(int) * a.n_beam, ctx.stream));
        WLK_HIP(hipMemsetAsync(a.attn_last, 0, sizeof(float) * a.n_beam * a.T, ctx.stream));
        return;
    }
    launch_align_zscore(ctx, a);
    const size_t lds = (size_t)a.n_align * a.T * sizeof(float);
    if (lds + 8192 + 1024 > 150 * 1024) {
        launch_align_argmax_plain(ctx, a);
        return;
    }
    KernelScope ks(ctx, "align_argmax");
    static std::atomic<bool> attr_set[64];   // launches come from several host threads
    int dev = 0;
    WLK_HIP(hipGetDevice(&dev));
    if (dev < 64 && !attr_set[dev].load(std::memory_order_acquire)) {
        WLK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(align_argmax_lds_kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
        attr_set[dev].store(true, std::memory_order_release);
    }
    hipLaunchKernelGGL(align_argmax_lds_kernel, dim3(a.n_beam), dim3(1024), lds, ctx.stream, a);
    WLK_HIP(hipGetLastError());
}

}  // namespace wlk
