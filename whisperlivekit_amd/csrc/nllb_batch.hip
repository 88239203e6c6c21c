// NLLB-200 / M2M-100: up to 8 DIFFERENT sentences in one launch chain (config 5 runs 8 translation sessions; a single-token
// step streams the decoder's layer weights and the tied vocabulary matrix once per call, so 8 sentences stepped one after
// another stream them 8 times).  nllb.hip's session holds one sentence - its rows are hypotheses of that sentence and all
// read one cross K/V and one source length.  Here a batch owns `n_slots` SLOTS, each one sentence in flight with
//
//   enc_out   [max_src][d]                      cross_kv  [max_src][dec_layers][k | v]   (the session's layout)
//   kcache / vcache  [dec_layers][max_tgt][d]    src_len, self_len
//
// and the batch owns the stacked work buffers, the row table, the stream and the step graphs.
//
//   encode(slots, ids, offsets)  the named slots' sentences concatenated: ONE embedding launch (positions restart inside
//                                every sentence), LayerNorm / GEMM / FFN once over all sum(S_i) rows, self-attention per
//                                segment (launch_sf_attention's n_seg: no score crosses a sentence), cross K/V projected
//                                over all rows and copied into each slot's own buffer.  Slots not named are untouched -
//                                they may be in the middle of a decode; that is what lets a new sentence take a freed slot.
//   step((slot, token) x R)      one decoder pass over R rows, any subset of the slots in any order: nl_decoder_layers'
//                                fused form (LayerNorm-fused weight-streaming GEMVs, the cache append riding in the qkv GEMV
//                                through GemmArgs::kv_rows, launch_decoder_self_attention_rows) with every per-row scalar
//                                (token, position, caches, cross K/V, SOURCE LENGTH) in a row table.  The host writes the
//                                table into a host-coherent block; the chain's first kernel reads it over the bus and
//                                leaves a device copy for the kernels behind it; the top-k kernel writes its results into
//                                host-coherent memory.  The chain is one graph per row count - and because no launch
//                                carries a length or an offset by value, a recording serves every later mix of sentences
//                                (the session's step graph carries the source length and is re-recorded per length:
//                                NlGraphSlot::src).
//
// Two kernels are new: the row-table embedding and the RAGGED cross-attention (every row its own key count, 1..512, read
// from the table).  The row table is common.h's StepRow - the type the GEMV's cache append and the self-attention
// launcher already index - with `content_len` holding the row's source length (its meaning for Whisper rows as well: the
// number of valid encoder positions).  fp32 throughout.
#include <algorithm>
#include <climits>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/wlk_hip.h"
#include "common.h"
#include "internal.h"
#include "nllb_internal.h"
#include "wave_ops.h"

namespace wlk {

constexpr int kNlBatchMaxRows = 8;         // rows of a stacked step = the weight-streaming GEMV's limit (gemv_applicable)
constexpr int kNlCrossMaxT = 512;          // == kSfMaxFrames, the bound nl_check_dims puts on max_src
static_assert(kNlCrossMaxT == kSfMaxFrames, "the encoder's attention and the ragged cross-attention share the source bound");
static_assert(kNlBatchMaxRows == kSfMaxSegments, "a stacked encode is one attention segment per slot");
static_assert(sizeof(StepRow) % 16 == 0, "the row table is copied in 4-byte words, rows stay 16-byte aligned");

struct NlSegTable {                         // by-value table of a stacked encode (never replayed from a graph)
    int n = 0;
    int start[kNlBatchMaxRows] = {0};       // first stacked row of segment s
};

// stacked ragged encode: x[r][:] = emb[tokens[r]][:] * scale + pos[pos0 + (r - start of r's sentence)][:]
__global__ __launch_bounds__(256) void nllb_embed_segments_kernel(const int* __restrict__ tokens, const float* __restrict__ emb,
                                                                  const float* __restrict__ pos, float scale, int pos0,
                                                                  NlSegTable sg, int d, float* __restrict__ x) {
    const int r = blockIdx.x;
    int first = 0;
#pragma unroll
    for (int s = 1; s < kNlBatchMaxRows; ++s) first = (s < sg.n && r >= sg.start[s]) ? sg.start[s] : first;
    const float4* e = reinterpret_cast<const float4*>(emb + (long)tokens[r] * d);
    const float4* p = reinterpret_cast<const float4*>(pos + (long)(pos0 + r - first) * d);
    float4* o = reinterpret_cast<float4*>(x + (long)r * d);
    for (int c = threadIdx.x; c < d / 4; c += 256) {
        const float4 ev = e[c], pv = p[c];
        o[c] = make_float4(ev.x * scale + pv.x, ev.y * scale + pv.y, ev.z * scale + pv.z, ev.w * scale + pv.w);
    }
}

// First kernel of a stacked step: workgroup r pulls row r of the table out of the host-coherent block (one uncached
// 4-byte read per lane, all in flight together), leaves it in the device copy for the kernels behind this one, and
// writes x[r][:] = emb[token_r][:] * scale + pos[pos0 + offset_r][:].
__global__ __launch_bounds__(256) void nllb_embed_rows_step_kernel(const StepRow* __restrict__ host_rows,
                                                                   StepRow* __restrict__ dev_rows, const float* __restrict__ emb,
                                                                   const float* __restrict__ pos, float scale, int pos0, int d,
                                                                   float* __restrict__ x) {
    constexpr int kRowWords = sizeof(StepRow) / 4;
    __shared__ __attribute__((aligned(16))) unsigned mine[kRowWords];
    const int tid = threadIdx.x, row = blockIdx.x;
    if (tid < kRowWords) {
        const unsigned w = __hip_atomic_load(reinterpret_cast<const unsigned*>(host_rows + row) + tid, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_SYSTEM);
        mine[tid] = w;
        reinterpret_cast<unsigned*>(dev_rows + row)[tid] = w;
    }
    __syncthreads();
    const StepRow* sr = reinterpret_cast<const StepRow*>(mine);
    const float4* e = reinterpret_cast<const float4*>(emb + (long)sr->token * d);
    const float4* p = reinterpret_cast<const float4*>(pos + (long)(pos0 + sr->offset) * d);
    float4* o = reinterpret_cast<float4*>(x + (long)row * d);
    for (int c = tid; c < d / 4; c += 256) {
        const float4 ev = e[c], pv = p[c];
        o[c] = make_float4(ev.x * scale + pv.x, ev.y * scale + pv.y, ev.z * scale + pv.z, ev.w * scale + pv.w);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Ragged decoder cross-attention of a stacked step: one 256-thread workgroup per (row, head); row r attends to the
// T_r = rows[r].content_len keys / values of ITS sentence (rows[r].cross_kv + kv_off, key stride ldkv), 1 <= T_r <= 512.
// launch_decoder_cross_attention takes one T by value and is shaped for Whisper's 1500 keys (key-parallel split + merge);
// a translation source is 5 .. 60 tokens and differs per row, so the whole head fits one workgroup pass:
//   scores   a 16-lane group reads one 256-byte key row (float4 per lane), a wave covers 4 keys per instruction, the 4
//            waves 16; 8 instructions (128 keys - every usual sentence) are in flight before the first dot is folded
//   softmax  scores in LDS, wave reductions + one LDS exchange (decoder_self_attention_kernel's order)
//   values   the same row mapping, the weights from LDS, 16 partial head rows merged through LDS
// Nothing is read at or past key T_r: lanes beyond it re-read key 0 and their scores are never stored.  A workgroup
// touches only its own row's operands, so a row's output bits do not depend on which other rows share the launch.
// ---------------------------------------------------------------------------------------------------------------------
//
// kAlign (align steps): a (row, head) whose rank in the layer's table head_rank[heads] is >= 0 also stores its
// normalised sc[0..T_r) - the weights the value pass multiplies by - to align_probs[rank][row][0..T_r) (row stride
// align_stride, kNlBatchMaxRows rows per rank), each thread the entries it has just normalised.  The attention output has
// the bits of the kAlign = false instantiation: the stores are the only difference.
template <bool kAlign>
__global__ __launch_bounds__(256) void nllb_cross_attention_ragged_kernel(const float* __restrict__ q,
                                                                          const StepRow* __restrict__ rows, long kv_off,
                                                                          long ldkv, int d, float* __restrict__ out,
                                                                          const int* __restrict__ head_rank,
                                                                          float* __restrict__ align_probs, int align_stride) {
    __shared__ float sc[kNlCrossMaxT];
    __shared__ float red[8];
    __shared__ __attribute__((aligned(16))) float part[16 * 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sub = lane & 15, kq = lane >> 4;
    const int row = blockIdx.x, head = blockIdx.y;
    const float4 q4 = *reinterpret_cast<const float4*>(q + (long)row * d + head * 64 + sub * 4);
    int T = rows[row].content_len;
    T = T < 1 ? 1 : (T > kNlCrossMaxT ? kNlCrossMaxT : T);      // the host checks it; a bad table must not leave the LDS rows
    const gcf_ptr kb = to_global(rows[row].cross_kv) + kv_off + head * 64 + sub * 4;
    const gcf_ptr vb = kb + d;

    float4 kk0[8], vv0[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int j = wave * 4 + 16 * u + kq;
        kk0[u] = ldg4(kb + (long)(j < T ? j : 0) * ldkv);
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int j = wave * 4 + 16 * u + kq;
        vv0[u] = ldg4(vb + (long)(j < T ? j : 0) * ldkv);
    }

    float mx = -INFINITY;
    for (int base = wave * 4; base < T; base += 16 * 8) {
        float4 kk[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int j = base + 16 * u + kq;
            if (base == wave * 4) kk[u] = kk0[u];
            else kk[u] = ldg4(kb + (long)(j < T ? j : 0) * ldkv);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int j = base + 16 * u + kq;
            float acc = 0.f;
            acc = fmaf(q4.x, kk[u].x, acc);
            acc = fmaf(q4.y, kk[u].y, acc);
            acc = fmaf(q4.z, kk[u].z, acc);
            acc = fmaf(q4.w, kk[u].w, acc);
            acc = row16_sum_1248(acc);
            if (j < T) {
                if (sub == 0) sc[j] = acc;
                mx = fmaxf(mx, acc);
            }
        }
    }
    mx = wave_max(mx);
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));      // (a wave without keys contributes -inf)
    float sum = 0.f;
    for (int j = tid; j < T; j += 256) {
        const float e = expf(sc[j] - mx);
        sc[j] = e;
        sum += e;
    }
    sum = wave_sum(sum);
    if (lane == 0) red[4 + wave] = sum;
    __syncthreads();
    sum = (red[4] + red[5]) + (red[6] + red[7]);
    if (kAlign) {
        const int rank = head_rank[head];
        float* keep = align_probs + ((long)(rank < 0 ? 0 : rank) * kNlBatchMaxRows + row) * align_stride;
        for (int j = tid; j < T; j += 256) {
            const float w = sc[j] / sum;
            sc[j] = w;
            if (rank >= 0) keep[j] = w;
        }
    } else {
        for (int j = tid; j < T; j += 256) sc[j] = sc[j] / sum;
    }
    __syncthreads();

    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int base = wave * 4; base < T; base += 16 * 8) {
        float4 vv[8];
        float ww[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int j = base + 16 * u + kq;
            const bool ok = j < T;
            if (base == wave * 4) vv[u] = vv0[u];
            else vv[u] = ldg4(vb + (long)(ok ? j : 0) * ldkv);
            ww[u] = ok ? sc[j] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            o.x = fmaf(ww[u], vv[u].x, o.x);
            o.y = fmaf(ww[u], vv[u].y, o.y);
            o.z = fmaf(ww[u], vv[u].z, o.z);
            o.w = fmaf(ww[u], vv[u].w, o.w);
        }
    }
    reinterpret_cast<float4*>(part)[(wave * 4 + kq) * 16 + sub] = o;
    __syncthreads();
    if (tid < 64) {
        float acc = 0.f;
#pragma unroll
        for (int s = 0; s < 16; ++s) acc += part[s * 64 + tid];
        out[(long)row * d + head * 64 + tid] = acc;
    }
}

// What the two launchers below refuse (std::invalid_argument).  lengths / head_rank (may be null): the host's copy of the
// table's content_len and of the rank table, where the caller has one; n_rank = the ranks align_probs holds.
static void nllb_cross_ragged_check(int n_rows, int d, int n_head, long kv_off, long ldkv, const int* lengths, bool align,
                                    const int* head_rank, int n_rank, int align_stride) {
    auto need = [](bool ok, const char* what) {
        if (!ok) throw std::invalid_argument(std::string("NLLB ragged cross-attention: ") + what);
    };
    need(n_rows >= 1 && n_head >= 1 && d == 64 * n_head, "rows >= 1 and d = 64 n_head");
    need(kv_off >= 0 && kv_off % 4 == 0 && ldkv % 4 == 0 && kv_off + 2L * d <= ldkv, "a key row does not hold k | v at kv_off");
    if (lengths)
        for (int r = 0; r < n_rows; ++r) need(lengths[r] >= 1 && lengths[r] <= kNlCrossMaxT, "a row has 1 .. 512 keys");
    if (!align) return;
    need(n_rows <= kNlBatchMaxRows && align_stride >= 1 && align_stride <= kNlCrossMaxT, "the alignment rows hold 8 rows of at most 512 positions");
    if (lengths)
        for (int r = 0; r < n_rows; ++r) need(lengths[r] <= align_stride, "a row has more keys than an alignment row holds");
    if (head_rank)
        for (int h = 0; h < n_head; ++h) need(head_rank[h] >= -1 && head_rank[h] < n_rank, "a head's rank lies outside the alignment rows");
}

static void launch_nllb_cross_attention_ragged(const LaunchCtx& ctx, const float* q, const StepRow* rows, long kv_off, long ldkv,
                                               float* out, int n_rows, int d, int n_head) {
    nllb_cross_ragged_check(n_rows, d, n_head, kv_off, ldkv, nullptr, false, nullptr, 0, 0);
    KernelScope ks(ctx, "nllb_cross_attention_ragged");
    hipLaunchKernelGGL(nllb_cross_attention_ragged_kernel<false>, dim3(n_rows, n_head), dim3(256), 0, ctx.stream, q, rows, kv_off,
                       ldkv, d, out, (const int*)nullptr, (float*)nullptr, 0);
    WLK_HIP(hipGetLastError());
}

// the same launch for an align step: n_rows <= kNlBatchMaxRows, head_rank = the layer's [n_head] rank table
static void launch_nllb_cross_attention_ragged_align(const LaunchCtx& ctx, const float* q, const StepRow* rows, long kv_off,
                                                     long ldkv, float* out, int n_rows, int d, int n_head, const int* head_rank,
                                                     float* align_probs, int align_stride) {
    if (n_rows > kNlBatchMaxRows || !head_rank || !align_probs || align_stride < 1 || align_stride > kNlCrossMaxT)
        throw std::invalid_argument("NLLB ragged cross-attention: the alignment rows hold 8 rows of at most 512 positions");
    nllb_cross_ragged_check(n_rows, d, n_head, kv_off, ldkv, nullptr, true, nullptr, 0, align_stride);
    KernelScope ks(ctx, "nllb_cross_attention_ragged_align");
    hipLaunchKernelGGL(nllb_cross_attention_ragged_kernel<true>, dim3(n_rows, n_head), dim3(256), 0, ctx.stream, q, rows, kv_off,
                       ldkv, d, out, head_rank, align_probs, align_stride);
    WLK_HIP(hipGetLastError());
}

// ---------------------------------------------------------------------------------------------------------------------
// Ragged AlignAtt read-out: nllb.hip's nllb_align_readout_kernel with every per-row scalar read per row.
// probs [n_align][.][stride] (head stride by value), one workgroup per row, two positions per thread:
//   S_r                 = rows[r].content_len (clamped to 1..min(stride, 512): a bad table must not leave the row)
//   lo_r | hi_r | limit_r = ctl[3 r .. 3 r + 2], a host-coherent block in a replayed step
//   p[j]  = (probs[0][r][j] + probs[1][r][j] + ... in rank order) * inv_n, j < S_r, written to p_out[r][j] (row stride `stride`)
//   pos / prob / mass as the session's kernel defines them: a thread takes its lower position first, a tie goes to the
//   lowest index, the mass is (w0 + w1) + (w2 + w3).  Nothing is read or written at or past S_r of a row.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void nllb_align_readout_rows_kernel(const float* __restrict__ probs, int n_align,
                                                                      long head_stride, int stride, float inv_n,
                                                                      const StepRow* __restrict__ rows, const int* __restrict__ ctl,
                                                                      float* __restrict__ p_out, int* __restrict__ pos,
                                                                      float* __restrict__ prob, float* __restrict__ mass) {
    __shared__ float red_v[4], red_m[4];
    __shared__ int red_i[4];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cap = stride < kNlCrossMaxT ? stride : kNlCrossMaxT;
    int S = rows[row].content_len;
    S = S < 1 ? 1 : (S > cap ? cap : S);
    const int lo = max(__hip_atomic_load(ctl + 3 * row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM), 0);
    const int hi = min(__hip_atomic_load(ctl + 3 * row + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM), S);
    const int limit = max(__hip_atomic_load(ctl + 3 * row + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM), 0);
    const float* base = probs + (long)row * stride;
    float bv = -INFINITY, tail = 0.f;
    int bi = INT_MAX;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int j = tid + half * 256;
        if (j < S) {
            float acc = 0.f;
            for (int a = 0; a < n_align; ++a) acc += base[a * head_stride + j];
            const float p = acc * inv_n;
            p_out[(long)row * stride + j] = p;
            if (j >= limit) tail += p;
            if (j >= lo && j < hi && p > bv) { bv = p; bi = j; }      // j ascends: an equal value keeps the lower position
        }
    }
    wave_argmax(bv, bi);
    tail = wave_sum(tail);
    if (lane == 0) { red_v[wave] = bv; red_i[wave] = bi; red_m[wave] = tail; }
    __syncthreads();
    if (tid == 0) {
        float v = red_v[0];
        int i = red_i[0];
        for (int w = 1; w < 4; ++w)
            if (red_v[w] > v || (red_v[w] == v && red_i[w] < i)) { v = red_v[w]; i = red_i[w]; }
        const bool found = i != INT_MAX;
        pos[row] = found ? i : -1;
        prob[row] = found ? v : 0.f;
        mass[row] = (red_m[0] + red_m[1]) + (red_m[2] + red_m[3]);
    }
}

void launch_nllb_align_readout_rows(const LaunchCtx& ctx, const float* probs, int n_align, long head_stride, int stride,
                                    int n_rows, const StepRow* rows, const int* ctl, float* p_out, int* pos, float* prob,
                                    float* mass) {
    if (n_align < 1 || n_align > kNlMaxAlign || n_rows < 1 || n_rows > kNlBatchMaxRows || stride < 1 || stride > kNlCrossMaxT ||
        head_stride < (long)n_rows * stride)
        throw std::invalid_argument("NLLB ragged alignment read-out: 1..64 heads, 1..8 rows, row stride 1..512");
    KernelScope ks(ctx, "nllb_align_readout_rows");
    hipLaunchKernelGGL(nllb_align_readout_rows_kernel, dim3(n_rows), dim3(256), 0, ctx.stream, probs, n_align, head_stride, stride,
                       1.0f / (float)n_align, rows, ctl, p_out, pos, prob, mass);
    WLK_HIP(hipGetLastError());
}

// ---------------------------------------------------------------------------------------------------------------------
// Draft verification (wlk_nllb_batch_verify): the arg-max of every candidate row, then one wave per slot that
// compares the picks with the draft.
//
// nllb_verify_pick_rows_kernel: grid (kNlPickSlices, rows).  A row of 256 206 logits is 1 MB - one workgroup per row would
// pull it through one CU - so a row is cut into kNlPickSlices slices of `per` (even) elements and workgroup (s, r) reads
// slice s of row r ONCE: thread t owns the element pairs (u * 256 + t) of every block of 256 * kNlPickLoads pairs, issues
// the kNlPickLoads loads of a block before it folds the first, and keeps the best (value, id) it has seen.  A greedy id
// needs no normaliser: no expf, no candidate list.  Order: value descending, id ascending - rank 0 of
// launch_logsoftmax_topk on the same row.
//   kVec2    n_vocab is even: every row and every slice starts 8-byte aligned (NOT 16: 256 206 * 4 = 1 024 824), a pair
//            is one 8-byte load.  Odd vocabularies (tests) take two 4-byte loads per pair.
// Nothing is read at or past the slice's end: a pair beyond it re-reads the slice's first pair and is never folded.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kNlVerifyChunk = 128;        // rows of logits a verify forms at a time (131 MB at NLLB's vocabulary)
constexpr int kNlPickLoads = 16;           // 8-byte loads a thread has in flight: 32 slices x 256 threads x 16 pairs = 262 144

__device__ __forceinline__ bool nl_pick_better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

// the fold of a row's partials, by one lane: all kNlPickSlices entries requested before the first comparison
__device__ __forceinline__ NlPick nl_pick_fold(const NlPick* __restrict__ parts, long row) {
    NlPick p[kNlPickSlices];
#pragma unroll
    for (int s = 0; s < kNlPickSlices; ++s) p[s] = parts[row * kNlPickSlices + s];
    NlPick b = p[0];
#pragma unroll
    for (int s = 1; s < kNlPickSlices; ++s)
        if (nl_pick_better(p[s].v, p[s].i, b.v, b.i)) b = p[s];
    return b;
}

template <bool kVec2>
__global__ __launch_bounds__(256) void nllb_verify_pick_rows_kernel(const float* __restrict__ logits, int n_vocab,
                                                                    NlPick* __restrict__ parts) {
    __shared__ float cand_v[4];
    __shared__ int cand_i[4];
    const int tid = threadIdx.x, slice = blockIdx.x, row = blockIdx.y;
    const int per = (((n_vocab + kNlPickSlices - 1) / kNlPickSlices) + 1) & ~1;
    const int lo = slice * per;
    const int hi = min(n_vocab, lo + per);
    const float* x = logits + (long)row * n_vocab;
    const int safe = lo < hi ? lo : 0;                 // (an empty trailing slice reads nothing: its loop does not run)
    float bv = -INFINITY;
    int bi = INT_MAX;
    for (int base = lo; base < hi; base += 2 * 256 * kNlPickLoads) {
        float2 v[kNlPickLoads];
#pragma unroll
        for (int u = 0; u < kNlPickLoads; ++u) {
            const int i = base + 2 * (u * 256 + tid);
            if (kVec2) {
                v[u] = *reinterpret_cast<const float2*>(x + (i < hi ? i : safe));      // hi is even: i < hi means i + 1 < hi
            } else {
                v[u].x = x[i < hi ? i : safe];
                v[u].y = x[i + 1 < hi ? i + 1 : safe];
            }
        }
#pragma unroll
        for (int u = 0; u < kNlPickLoads; ++u) { pin_loaded(v[u].x); pin_loaded(v[u].y); }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < kNlPickLoads; ++u) {
            const int i = base + 2 * (u * 256 + tid);
            if (i < hi && nl_pick_better(v[u].x, i, bv, bi)) { bv = v[u].x; bi = i; }
            if (i + 1 < hi && nl_pick_better(v[u].y, i + 1, bv, bi)) { bv = v[u].y; bi = i + 1; }
        }
    }
    wave_argmax(bv, bi);
    if ((tid & 63) == 0) { cand_v[tid >> 6] = bv; cand_i[tid >> 6] = bi; }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (nl_pick_better(cand_v[w], cand_i[w], bv, bi)) { bv = cand_v[w]; bi = cand_i[w]; }
        NlPick out;
        out.v = bv;
        out.i = bi;
        parts[(long)row * kNlPickSlices + slice] = out;
    }
}

void launch_nllb_verify_pick_rows(const LaunchCtx& ctx, const float* logits, int n_vocab, int n_rows, NlPick* parts) {
    if (n_vocab < 1 || n_rows < 1 || n_rows > 65535) throw std::invalid_argument("NLLB verify pick: n_vocab >= 1, 1..65535 rows");
    KernelScope ks(ctx, "nllb_verify_pick_rows", 0.0, 4.0 * n_rows * (double)n_vocab);
    if (n_vocab % 2 == 0)
        hipLaunchKernelGGL(nllb_verify_pick_rows_kernel<true>, dim3(kNlPickSlices, n_rows), dim3(256), 0, ctx.stream, logits, n_vocab, parts);
    else
        hipLaunchKernelGGL(nllb_verify_pick_rows_kernel<false>, dim3(kNlPickSlices, n_rows), dim3(256), 0, ctx.stream, logits, n_vocab, parts);
    WLK_HIP(hipGetLastError());
}

// diagnostics: the fold alone, one lane per row
__global__ __launch_bounds__(64) void nllb_verify_fold_rows_kernel(const NlPick* __restrict__ parts, int n_rows,
                                                                   const int* __restrict__ targets, int* __restrict__ picks,
                                                                   int* __restrict__ match) {
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= n_rows) return;
    const NlPick b = nl_pick_fold(parts, r);
    picks[r] = b.i;
    match[r] = b.i == targets[r] ? 1 : 0;
}

void launch_nllb_verify_fold_rows(const LaunchCtx& ctx, const NlPick* parts, int n_rows, const int* targets, int* picks, int* match) {
    if (n_rows < 1) throw std::invalid_argument("NLLB verify fold: rows >= 1");
    KernelScope ks(ctx, "nllb_verify_fold_rows");
    hipLaunchKernelGGL(nllb_verify_fold_rows_kernel, dim3((n_rows + 63) / 64), dim3(64), 0, ctx.stream, parts, n_rows, targets, picks, match);
    WLK_HIP(hipGetLastError());
}

// One wave per slot behind the picks.  Slot i's rows are row0[i] .. row0[i] + P[i] of the stacked table (P = 2 + n_d); the
// logits of row 1 + j predict draft token d_j = the token of row 2 + j, and the logits of the last row what follows the draft.
//   pick_j = nl_pick_fold of row row0 + 1 + j, j = 0 .. n_d (lane = j mod 64, 64 positions a round)
//   k      = the first j with j == n_d or pick_j != d_j: a ballot over the miss flags, the first set bit
//   res[2 i] = k, res[2 i + 1] = pick_k - plain stores by the lane that holds position k, into host-coherent memory
struct NlVerifySlots {
    int n = 0;
    int row0[kNlBatchMaxRows] = {0}, P[kNlBatchMaxRows] = {0};
};
__global__ __launch_bounds__(64) void nllb_verify_accept_kernel(const NlPick* __restrict__ parts, const StepRow* __restrict__ rows,
                                                                NlVerifySlots sl, int* __restrict__ res) {
    const int slot = blockIdx.x, lane = threadIdx.x;
    int r0 = 0, P = 2;
#pragma unroll
    for (int s = 0; s < kNlBatchMaxRows; ++s)
        if (s == slot) { r0 = sl.row0[s]; P = sl.P[s]; }
    const int n_d = P - 2;
    for (int base = 0; base <= n_d; base += 64) {
        const int j = base + lane;
        const bool live = j <= n_d;
        const int draft = rows[r0 + (j < n_d ? 2 + j : 0)].token;
        const NlPick pick = nl_pick_fold(parts, r0 + 1 + (live ? j : 0));
        const bool miss = !(j < n_d && pick.i == draft);
        const unsigned long long m = __ballot(miss);
        if (m != 0ull) {
            const int k = base + __ffsll((long long)m) - 1;      // k <= n_d: position n_d always misses
            if (j == k) {
                res[2 * slot] = k;
                res[2 * slot + 1] = pick.i;
            }
            break;
        }
    }
}

struct NlBatchSlot {
    float *enc_out = nullptr, *cross_kv = nullptr, *kcache = nullptr, *vcache = nullptr;
    int src_len = 0, self_len = 0;
    bool encoded = false;
    int logits_row = -1;       // row of the latest step's logits that is this slot's, -1: the slot was not in it
    int align_row = -1;        // row of the latest ALIGN step's p that is this slot's, -1: the slot was not in it
};

}  // namespace wlk

using namespace wlk;

struct wlk_nllb_batch : NlOwner {
    // graphs[]: the plain step by row count, then the align step by row count (dropped with the head set)
    enum { kStepGraph = 0, kAlignGraph = kNlBatchMaxRows + 1, kGraphs = 2 * (kNlBatchMaxRows + 1) };
    wlk_nllb_batch() : NlOwner(kGraphs) {}
    int n_slots = 0;
    std::vector<NlBatchSlot> slots;
    // stacked encode (n_slots x max_src rows)
    float *ex = nullptr, *eh = nullptr, *eqkv = nullptr, *eatt = nullptr, *ewide = nullptr, *enc_stack = nullptr, *xkv_stack = nullptr;
    int* enc_tokens = nullptr;
    // stacked step (up to 8 rows; fused only: no h)
    NlDecWs ws{};
    float* logits = nullptr;
    void* topk_scratch = nullptr;
    StepRow* rows_dev = nullptr;         // the device copy of the row table, written by the chain's first kernel
    StepRow* probe_rows_dev = nullptr;   // wlk_nllb_batch_cross_attention's own table
    StepRow* rows_host = nullptr;        // pinned + mapped: [8] rows
    StepRow* rows_host_dev = nullptr;    // the same block as the device sees it
    float* vals_host = nullptr;          // pinned + mapped: top-k results written by the top-k kernel itself
    int* ids_host = nullptr;
    float* vals_dev = nullptr;
    int* ids_dev = nullptr;
    // AlignAtt steps (wlk_nllb_batch_step_align); nothing below is allocated before the first align step
    int n_align = 0;
    std::vector<int> head_rank;          // [dec_layers][heads]: rank of the (layer, head) pair or -1, as set
    bool head_rank_stale = false;        // head_rank_dev does not hold head_rank yet
    int* head_rank_dev = nullptr;
    float* align_probs = nullptr;        // [kNlMaxAlign][8][max_src]: the selected heads' softmax rows of the latest align step
    float* align_p = nullptr;            // [8][max_src]: their mean
    int* align_host = nullptr;           // pinned + mapped: [8] lo | hi | limit, then [8] position, [8] probability, [8] tail mass
    int* align_host_dev = nullptr;
    uint64_t align_steps = 0, align_captures = 0;
    // stacked prompt prefill (wlk_nllb_batch_prefill): n_slots x max_tgt rows, allocated by the first prefill
    NlDecWs pws{};
    StepRow *prefill_stage = nullptr, *prefill_rows = nullptr;    // the uploaded table and the copy the embedding leaves
    // draft verification (wlk_nllb_batch_verify); nothing below is allocated before the first verify
    float* vlogits = nullptr;            // [kNlVerifyChunk][vocab]: one chunk of candidate rows' logits, reused chunk by chunk
    NlPick* vparts = nullptr;            // [n_slots x max_tgt][kNlPickSlices]: every candidate row's slice partials
    int *vres_host = nullptr, *vres_dev = nullptr;      // pinned + mapped: [8] accepted | next token
    uint64_t verify_passes = 0, verify_draft = 0, verify_accepted = 0;
};

namespace wlk {

static void nlb_encode(wlk_nllb_batch* b, const NlSegTable& sg, const int* len, int total) {
    wlk_nllb* m = b->m;
    const wlk_nllb_dims& D = m->D;
    hipLaunchKernelGGL(nllb_embed_segments_kernel, dim3(total), dim3(256), 0, b->stream, b->enc_tokens, m->emb, m->pos, D.embed_scale,
                       D.pad_id + 1, sg, D.d_model, b->ex);
    WLK_HIP(hipGetLastError());
    SfAttnArgs seg;
    seg.n_seg = sg.n;
    for (int s = 0; s < sg.n; ++s) {
        seg.seg_start[s] = sg.start[s]; seg.seg_T[s] = len[s];
        seg.T = std::max(seg.T, len[s]);
    }
    nl_encoder_layers(b->ctx(), m, b->ex, b->eh, b->eqkv, b->eatt, b->ewide, b->enc_stack, b->xkv_stack, total, seg);
}

// Row-table addressing of the decoder layers: row r's caches ([dec_layers][max_tgt][d]), position, cross K/V and SOURCE
// LENGTH come from rows[r].  align: the selected heads leave their softmax rows in align_probs.
struct NlRowsAddr {
    const wlk_nllb_batch* b;
    const StepRow* rows;
    int R;
    bool align;
    const wlk_nllb_dims& D() const { return b->m->D; }
    long layer_off(int l) const { return (long)l * D().max_tgt * D().d_model; }
    void kv_rider(GemmArgs& g, int l) const {
        g.kv_rows = rows; g.kv_layer_off = layer_off(l); g.kv_d = D().d_model; g.kv_ctx = D().max_tgt;
    }
    void append(const LaunchCtx& c, const float* qkv, int l) const { launch_kv_append_rows(c, qkv, rows, layer_off(l), R, D().d_model); }
    void self_attention(const LaunchCtx& c, const float* qkv, float* att, int l) const {
        launch_decoder_self_attention_rows(c, qkv, rows, layer_off(l), att, R, D().d_model, D().heads, D().max_tgt);
    }
    void cross_attention(const LaunchCtx& c, const float* q, float* att, int l) const {
        const int d = D().d_model, H = D().heads;
        const long kv_off = (long)l * 2 * d, ldkv = (long)D().dec_layers * 2 * d;
        if (align)
            launch_nllb_cross_attention_ragged_align(c, q, rows, kv_off, ldkv, att, R, d, H, b->head_rank_dev + (size_t)l * H,
                                                     b->align_probs, D().max_src);
        else
            launch_nllb_cross_attention_ragged(c, q, rows, kv_off, ldkv, att, R, d, H);
    }
};

// embed .. logits .. top-k of R stacked rows; every per-row scalar comes from the row table.  align: the selected heads
// leave their softmax rows in align_probs and the ragged read-out follows the top-k (windows and results in align_host)
static void nlb_step_chain(wlk_nllb_batch* b, int R, int k, bool align = false) {
    wlk_nllb* m = b->m;
    const wlk_nllb_dims& D = m->D;
    const LaunchCtx c = b->ctx();
    hipLaunchKernelGGL(nllb_embed_rows_step_kernel, dim3(R), dim3(256), 0, b->stream, b->rows_host_dev, b->rows_dev, m->emb,
                       m->pos, D.embed_scale, D.pad_id + 1, D.d_model, b->ws.x);
    WLK_HIP(hipGetLastError());
    nl_decoder_layers(c, m, b->ws, R, /*fused=*/true, NlRowsAddr{b, b->rows_dev, R, align});
    nl_logits(c, m, /*fused=*/true, b->ws.x, R, 1, nullptr, b->logits);
    // results straight into the host-coherent block: no copy node behind the graph
    launch_logsoftmax_topk(c, b->logits, D.vocab, R, k, b->vals_dev, b->ids_dev, b->topk_scratch, nullptr, nullptr, nullptr, 0);
    if (align) {
        int* res = b->align_host_dev + 3 * kNlBatchMaxRows;
        launch_nllb_align_readout_rows(c, b->align_probs, b->n_align, (long)kNlBatchMaxRows * D.max_src, D.max_src, R, b->rows_dev,
                                       b->align_host_dev, b->align_p, res, reinterpret_cast<float*>(res + kNlBatchMaxRows),
                                       reinterpret_cast<float*>(res + 2 * kNlBatchMaxRows));
    }
}

// Stacked prompt prefill: N rows, row i = (slot, token, position) of prefill_rows - no final LayerNorm, no logits.  Row p of
// a slot sees cache positions 0..p of that slot: every layer appends ALL rows' keys / values in front of its attention launch.
static void nlb_prefill_chain(wlk_nllb_batch* b, int N) {
    wlk_nllb* m = b->m;
    const wlk_nllb_dims& D = m->D;
    hipLaunchKernelGGL(nllb_embed_rows_step_kernel, dim3(N), dim3(256), 0, b->stream, b->prefill_stage, b->prefill_rows, m->emb,
                       m->pos, D.embed_scale, D.pad_id + 1, D.d_model, b->pws.x);
    WLK_HIP(hipGetLastError());
    nl_decoder_layers(b->ctx(), m, b->pws, N, /*fused=*/false, NlRowsAddr{b, b->prefill_rows, N, false});
}

static StepRow nlb_row(const wlk_nllb_batch* b, int slot, int token) {
    const NlBatchSlot& s = b->slots[slot];
    StepRow r{};
    r.kcache = s.kcache; r.vcache = s.vcache; r.cross_kv = s.cross_kv; r.ring = nullptr;
    r.token = token; r.offset = s.self_len; r.content_len = s.src_len;
    return r;
}

// slots[n] in range and pairwise different
static int nlb_check_slots(const wlk_nllb_batch* b, const int32_t* slots, int n) {
    unsigned seen = 0;
    for (int i = 0; i < n; ++i) {
        if (slots[i] < 0 || slots[i] >= b->n_slots) return nl_fail(WLK_ERR_ARG, "NLLB batch: slot index out of range");
        if (seen & (1u << slots[i])) return nl_fail(WLK_ERR_ARG, "NLLB batch: a slot is named twice in one call");
        seen |= 1u << slots[i];
    }
    return WLK_OK;
}

// Host checks of a stacked prompt pass (prefill: min_len 1, verify: min_len 2) and its row table: row t = (slot, token,
// position inside the slot's prompt).  Refuses before anything is launched or changed.
static int nlb_prompt_table(const wlk_nllb_batch* b, const char* who, const int32_t* slots, const int64_t* ids, const int32_t* offsets,
                            int n, int min_len, std::vector<StepRow>& table) {
    const std::string w = who;
    if (n < 1 || n > b->n_slots) return nl_fail(WLK_ERR_ARG, w + ": 1..n_slots prompts per call");
    if (int rc = nlb_check_slots(b, slots, n)) return rc;
    const wlk_nllb_dims& D = b->m->D;
    if (offsets[0] != 0) return nl_fail(WLK_ERR_ARG, w + ": prompt_offsets must start at 0");
    for (int i = 0; i < n; ++i) {
        const NlBatchSlot& s = b->slots[slots[i]];
        if (!s.encoded) return nl_fail(WLK_ERR_STATE, w + " on a slot that is not encoded");
        if (s.self_len != 0) return nl_fail(WLK_ERR_STATE, w + " on a slot that already holds target tokens");
        const long pi = (long)offsets[i + 1] - offsets[i];
        if (pi < min_len) return nl_fail(WLK_ERR_ARG, w + (min_len == 1 ? ": every prompt needs at least one token"
                                                                        : ": needs the decoder start and the forced first token in front of the draft"));
        if (pi > D.max_tgt - 1) return nl_fail(WLK_ERR_CAPACITY, w + ": a prompt leaves no room for a step");
    }
    const int total = offsets[n];
    if (int rc = nl_check_tokens(D, ids, total)) return rc;
    table.resize((size_t)total);
    for (int i = 0; i < n; ++i)
        for (int t = offsets[i]; t < offsets[i + 1]; ++t) {
            table[t] = nlb_row(b, slots[i], (int)ids[t]);
            table[t].offset = t - offsets[i];
        }
    return WLK_OK;
}

// the prefill workspace (allocated by the first stacked prompt pass) and the table's upload; the stream is idle on entry
static void nlb_prompt_upload(wlk_nllb_batch* b, const std::vector<StepRow>& table) {
    const wlk_nllb_dims& D = b->m->D;
    if (!b->prefill_rows) {
        const size_t d = D.d_model, N = (size_t)b->n_slots * D.max_tgt;
        b->pws = NlDecWs{b->alloc<float>(N * d), b->alloc<float>(N * d), b->alloc<float>(N * 3 * d), b->alloc<float>(N * d),
                         b->alloc<float>(N * d), b->alloc<float>(N * D.ffn)};
        b->prefill_stage = b->alloc<StepRow>(N);
        b->prefill_rows = b->alloc<StepRow>(N);
    }
    WLK_HIP(hipMemcpyAsync(b->prefill_stage, table.data(), table.size() * sizeof(StepRow), hipMemcpyHostToDevice, b->stream));
    WLK_HIP(hipStreamSynchronize(b->stream));           // `table` is pageable
}

}  // namespace wlk

extern "C" {

int wlk_nllb_batch_create(wlk_nllb* m, int n_slots, wlk_nllb_batch** out) {
    if (!m || !out) return nl_fail(WLK_ERR_ARG, "NULL argument");
    if (!m->finalized) return nl_fail(WLK_ERR_STATE, "NLLB model not finalized");
    if (n_slots < 1 || n_slots > kNlBatchMaxRows) return nl_fail(WLK_ERR_ARG, "NLLB batch: 1..8 slots");
    if (!gemv_applicable(std::min(n_slots, kNlBatchMaxRows), m->D.d_model))
        return nl_fail(WLK_ERR_ARG, "NLLB batch: the model is too wide for that many stacked single-token rows");
    return nl_guarded([&]() {
        WLK_HIP(hipSetDevice(m->device));
        auto b = std::make_unique<wlk_nllb_batch>();
        b->m = m;
        b->n_slots = n_slots;
        WLK_HIP(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
        const wlk_nllb_dims& D = m->D;
        const size_t d = D.d_model, f = D.ffn, S = D.max_src, Tt = D.max_tgt, L = D.dec_layers, Smax = S * n_slots, R = kNlBatchMaxRows;
        b->slots.resize(n_slots);
        for (auto& s : b->slots) {
            s.enc_out = b->alloc<float>(S * d);
            s.cross_kv = b->alloc<float>(S * L * 2 * d);
            s.kcache = b->alloc<float>(L * Tt * d);
            s.vcache = b->alloc<float>(L * Tt * d);
        }
        b->ex = b->alloc<float>(Smax * d); b->eh = b->alloc<float>(Smax * d); b->eqkv = b->alloc<float>(Smax * 3 * d);
        b->eatt = b->alloc<float>(Smax * d); b->ewide = b->alloc<float>(Smax * f); b->enc_stack = b->alloc<float>(Smax * d);
        b->xkv_stack = b->alloc<float>(Smax * L * 2 * d);
        b->enc_tokens = b->alloc<int>(Smax);
        b->ws = NlDecWs{b->alloc<float>(R * d), nullptr, b->alloc<float>(R * 3 * d), b->alloc<float>(R * d), b->alloc<float>(R * d),
                        b->alloc<float>(R * f)};
        b->logits = b->alloc<float>(R * D.vocab);
        b->topk_scratch = b->alloc<char>(topk_scratch_bytes(R));
        b->rows_dev = b->alloc<StepRow>(R);
        b->probe_rows_dev = b->alloc<StepRow>(R);
        b->mapped(R, &b->rows_host, &b->rows_host_dev);
        b->mapped(R * 8, &b->vals_host, &b->vals_dev);
        b->mapped(R * 8, &b->ids_host, &b->ids_dev);
        *out = b.release();
        return WLK_OK;
    });
}

int wlk_nllb_batch_destroy(wlk_nllb_batch* b) {
    delete b;        // ~wlk_nllb_batch releases the stream, graphs and buffers
    return WLK_OK;
}

int wlk_nllb_batch_encode(wlk_nllb_batch* b, const int32_t* slots, const int64_t* src_ids, const int32_t* src_offsets, int32_t n) {
    if (!b || !slots || !src_ids || !src_offsets) return nl_fail(WLK_ERR_ARG, "NULL argument");
    if (n < 1 || n > b->n_slots) return nl_fail(WLK_ERR_ARG, "NLLB batch encode: 1..n_slots sentences per call");
    if (int rc = nlb_check_slots(b, slots, n)) return rc;
    const wlk_nllb_dims& D = b->m->D;
    if (src_offsets[0] != 0) return nl_fail(WLK_ERR_ARG, "NLLB batch encode: src_offsets must start at 0");
    NlSegTable sg;
    int len[kNlBatchMaxRows] = {0};
    sg.n = n;
    for (int i = 0; i < n; ++i) {
        const long li = (long)src_offsets[i + 1] - src_offsets[i];
        if (li < 1 || li > D.max_src) return nl_fail(WLK_ERR_CAPACITY, "source length out of range");
        sg.start[i] = src_offsets[i];
        len[i] = (int)li;
    }
    const int total = src_offsets[n];
    if (int rc = nl_check_tokens(D, src_ids, total, "padding inside a sentence is not supported (sentences are stacked, not padded)")) return rc;
    const std::vector<int> stage(src_ids, src_ids + total);
    return nl_guarded([&]() {
        WLK_HIP(hipSetDevice(b->m->device));
        WLK_HIP(hipStreamSynchronize(b->stream));
        WLK_HIP(hipMemcpyAsync(b->enc_tokens, stage.data(), (size_t)total * sizeof(int), hipMemcpyHostToDevice, b->stream));
        WLK_HIP(hipStreamSynchronize(b->stream));           // `stage` is pageable
        for (int i = 0; i < n; ++i) b->slots[slots[i]].encoded = false;      // a failure below leaves them unusable, not stale
        nlb_encode(b, sg, len, total);
        const size_t d = D.d_model, ld = (size_t)D.dec_layers * 2 * d;
        for (int i = 0; i < n; ++i) {
            NlBatchSlot& s = b->slots[slots[i]];
            WLK_HIP(hipMemcpyAsync(s.enc_out, b->enc_stack + (size_t)sg.start[i] * d, (size_t)len[i] * d * sizeof(float),
                                   hipMemcpyDeviceToDevice, b->stream));
            WLK_HIP(hipMemcpyAsync(s.cross_kv, b->xkv_stack + (size_t)sg.start[i] * ld, (size_t)len[i] * ld * sizeof(float),
                                   hipMemcpyDeviceToDevice, b->stream));
        }
        for (int i = 0; i < n; ++i) {
            NlBatchSlot& s = b->slots[slots[i]];
            s.src_len = len[i];
            s.self_len = 0;
            s.encoded = true;
            s.logits_row = -1;
            s.align_row = -1;
        }
        return WLK_OK;
    });
}

int wlk_nllb_batch_step(wlk_nllb_batch* b, const int32_t* slots, const int64_t* tokens, int32_t n_rows, int32_t k, float* logprobs,
                        int32_t* ids) {
    if (!b || !slots || !tokens || !logprobs || !ids) return nl_fail(WLK_ERR_ARG, "NULL argument");
    if (n_rows < 1 || n_rows > kNlBatchMaxRows || n_rows > b->n_slots)
        return nl_fail(WLK_ERR_ARG, "NLLB batch step: 1..min(8, n_slots) rows, at most one per slot");
    if (k < 1 || k > 8) return nl_fail(WLK_ERR_ARG, "k must be 1..8 (the top-k kernel's limit)");
    if (int rc = nlb_check_slots(b, slots, n_rows)) return rc;
    const wlk_nllb_dims& D = b->m->D;
    for (int r = 0; r < n_rows; ++r) {
        const NlBatchSlot& s = b->slots[slots[r]];
        if (!s.encoded) return nl_fail(WLK_ERR_STATE, "NLLB batch step on a slot that is not encoded");
        if (s.self_len + 1 > D.max_tgt) return nl_fail(WLK_ERR_CAPACITY, "target context exceeded");
        if (int rc = nl_check_tokens(D, tokens + r, 1)) return rc;
    }
    return nl_guarded([&]() {
        WLK_HIP(hipSetDevice(b->m->device));
        WLK_HIP(hipStreamSynchronize(b->stream));           // the previous step's readers of the host block are done
        for (int r = 0; r < n_rows; ++r) b->rows_host[r] = nlb_row(b, slots[r], (int)tokens[r]);
        nl_replay(b->stream, b->graphs[b->kStepGraph + n_rows], k, 0, [&] { nlb_step_chain(b, n_rows, k); });
        std::memcpy(logprobs, b->vals_host, (size_t)n_rows * k * sizeof(float));
        std::memcpy(ids, b->ids_host, (size_t)n_rows * k * sizeof(int));
        for (auto& s : b->slots) s.logits_row = -1;
        for (int r = 0; r < n_rows; ++r) {
            NlBatchSlot& s = b->slots[slots[r]];
            s.self_len += 1;
            s.logits_row = r;
        }
        return WLK_OK;
    });
}

int wlk_nllb_batch_set_align(wlk_nllb_batch* b, const int32_t* layer_head_pairs, int32_t n) {
    if (!b || (n > 0 && !layer_head_pairs)) return nl_fail(WLK_ERR_ARG, "NULL argument");
    if (n < 0 || n > kNlMaxAlign) return nl_fail(WLK_ERR_ARG, "wlk_nllb_batch_set_align: 0..64 (layer, head) pairs");
    std::vector<int> rank;
    if (int rc = nl_head_rank(b->m->D, layer_head_pairs, n, rank)) return rc;
    return nl_guarded([&]() {
        bool recorded = false;
        for (int r = 0; r <= kNlBatchMaxRows; ++r) recorded = recorded || b->graphs[b->kAlignGraph + r].exec;
        if (recorded) {                      // a recording carries the head count by value
            WLK_HIP(hipSetDevice(b->m->device));
            WLK_HIP(hipStreamSynchronize(b->stream));
            for (int r = 0; r <= kNlBatchMaxRows; ++r) b->graphs[b->kAlignGraph + r].drop();
        }
        for (auto& s : b->slots) s.align_row = -1;
        b->head_rank = std::move(rank);      // uploaded by the next align step: nothing is allocated here
        b->head_rank_stale = true;
        b->n_align = n;
        return WLK_OK;
    });
}

int wlk_nllb_batch_step_align(wlk_nllb_batch* b, const int32_t* slots, const int64_t* tokens, int32_t n_rows, int32_t k,
                              const int32_t* lo, const int32_t* hi, const int32_t* limit, float* logprobs, int32_t* ids,
                              int32_t* align_pos, float* align_prob, float* tail_mass) {
    if (!b || !slots || !tokens || !lo || !hi || !limit || !logprobs || !ids || !align_pos || !align_prob || !tail_mass)
        return nl_fail(WLK_ERR_ARG, "NULL argument");
    if (n_rows < 1 || n_rows > kNlBatchMaxRows || n_rows > b->n_slots)
        return nl_fail(WLK_ERR_ARG, "NLLB batch step: 1..min(8, n_slots) rows, at most one per slot");
    if (k < 1 || k > 8) return nl_fail(WLK_ERR_ARG, "k must be 1..8 (the top-k kernel's limit)");
    if (int rc = nlb_check_slots(b, slots, n_rows)) return rc;
    if (b->n_align < 1) return nl_fail(WLK_ERR_STATE, "wlk_nllb_batch_step_align before wlk_nllb_batch_set_align");
    const wlk_nllb_dims& D = b->m->D;
    // what the two align launchers would refuse is refused here: nothing may throw once the stream is capturing
    if (b->n_align > kNlMaxAlign || D.max_src < 1 || D.max_src > kNlCrossMaxT)
        return nl_fail(WLK_ERR_ARG, "wlk_nllb_batch_step_align: the alignment rows hold 64 heads of at most 512 positions");
    for (int r = 0; r < n_rows; ++r) {
        const NlBatchSlot& s = b->slots[slots[r]];
        if (!s.encoded) return nl_fail(WLK_ERR_STATE, "NLLB batch step on a slot that is not encoded");
        if (s.self_len == 0) return nl_fail(WLK_ERR_STATE, "wlk_nllb_batch_step_align before the slot's decoder prompt (prefill or step first)");
        if (s.self_len + 1 > D.max_tgt) return nl_fail(WLK_ERR_CAPACITY, "target context exceeded");
        if (int rc = nl_check_tokens(D, tokens + r, 1)) return rc;
        if (lo[r] < 0 || hi[r] > s.src_len || limit[r] < 0 || limit[r] > s.src_len)
            return nl_fail(WLK_ERR_ARG, "wlk_nllb_batch_step_align: needs 0 <= lo, hi <= src_len and 0 <= limit <= src_len in every row");
    }
    return nl_guarded([&]() {
        WLK_HIP(hipSetDevice(b->m->device));
        WLK_HIP(hipStreamSynchronize(b->stream));           // the previous step's readers of the host blocks are done
        constexpr int R8 = kNlBatchMaxRows;
        if (!b->align_host) {
            b->head_rank_dev = b->alloc<int>((size_t)D.dec_layers * D.heads);
            b->align_probs = b->alloc<float>((size_t)kNlMaxAlign * R8 * D.max_src);
            b->align_p = b->alloc<float>((size_t)R8 * D.max_src);
            b->mapped(6 * R8, &b->align_host, &b->align_host_dev);
        }
        if (b->head_rank_stale) {
            WLK_HIP(hipMemcpyAsync(b->head_rank_dev, b->head_rank.data(), b->head_rank.size() * sizeof(int), hipMemcpyHostToDevice,
                                   b->stream));
            WLK_HIP(hipStreamSynchronize(b->stream));
            b->head_rank_stale = false;
        }
        for (int r = 0; r < n_rows; ++r) {
            b->rows_host[r] = nlb_row(b, slots[r], (int)tokens[r]);
            b->align_host[3 * r] = lo[r]; b->align_host[3 * r + 1] = hi[r]; b->align_host[3 * r + 2] = limit[r];
        }
        if (nl_replay(b->stream, b->graphs[b->kAlignGraph + n_rows], k, 0, [&] { nlb_step_chain(b, n_rows, k, /*align=*/true); }))
            b->align_captures += 1;
        std::memcpy(logprobs, b->vals_host, (size_t)n_rows * k * sizeof(float));
        std::memcpy(ids, b->ids_host, (size_t)n_rows * k * sizeof(int));
        std::memcpy(align_pos, b->align_host + 3 * R8, (size_t)n_rows * sizeof(int));
        std::memcpy(align_prob, b->align_host + 4 * R8, (size_t)n_rows * sizeof(float));
        std::memcpy(tail_mass, b->align_host + 5 * R8, (size_t)n_rows * sizeof(float));
        for (auto& s : b->slots) s.logits_row = s.align_row = -1;
        for (int r = 0; r < n_rows; ++r) {
            NlBatchSlot& s = b->slots[slots[r]];
            s.self_len += 1;
            s.logits_row = s.align_row = r;
        }
        b->align_steps += 1;
        return WLK_OK;
    });
}

int wlk_nllb_batch_align_stats(wlk_nllb_batch* b, uint64_t* align_steps, uint64_t* graph_captures) {
    if (!b || !align_steps || !graph_captures) return nl_fail(WLK_ERR_ARG, "NULL argument");
    *align_steps = b->align_steps;
    *graph_captures = b->align_captures;
    return WLK_OK;
}

int wlk_nllb_batch_prefill(wlk_nllb_batch* b, const int32_t* slots, const int64_t* prompt_ids, const int32_t* prompt_offsets,
                           int32_t n) {
    if (!b || !slots || !prompt_ids || !prompt_offsets) return nl_fail(WLK_ERR_ARG, "NULL argument");
    std::vector<StepRow> table;
    if (int rc = nlb_prompt_table(b, "NLLB batch prefill", slots, prompt_ids, prompt_offsets, n, 1, table)) return rc;
    const int total = prompt_offsets[n];
    return nl_guarded([&]() {
        WLK_HIP(hipSetDevice(b->m->device));
        WLK_HIP(hipStreamSynchronize(b->stream));
        nlb_prompt_upload(b, table);
        nlb_prefill_chain(b, total);
        WLK_HIP(hipStreamSynchronize(b->stream));
        for (int i = 0; i < n; ++i) {
            NlBatchSlot& s = b->slots[slots[i]];
            s.self_len = prompt_offsets[i + 1] - prompt_offsets[i];
            s.logits_row = -1;
        }
        return WLK_OK;
    });
}

int wlk_nllb_batch_verify(wlk_nllb_batch* b, const int32_t* slots, const int64_t* ids, const int32_t* offsets, int32_t n,
                          int32_t* accepted, int64_t* next_token) {
    if (!b || !slots || !ids || !offsets || !accepted || !next_token) return nl_fail(WLK_ERR_ARG, "NULL argument");
    std::vector<StepRow> table;
    if (int rc = nlb_prompt_table(b, "NLLB batch verify", slots, ids, offsets, n, 2, table)) return rc;
    const wlk_nllb_dims& D = b->m->D;
    const int total = offsets[n];
    NlVerifySlots sl;
    sl.n = n;
    for (int i = 0; i < n; ++i) { sl.row0[i] = offsets[i]; sl.P[i] = offsets[i + 1] - offsets[i]; }
    return nl_guarded([&]() {
        WLK_HIP(hipSetDevice(b->m->device));
        WLK_HIP(hipStreamSynchronize(b->stream));
        if (!b->vres_host) {                 // (the last of the three: a failed allocation is tried again by the next call)
            b->vlogits = b->alloc<float>((size_t)kNlVerifyChunk * D.vocab);
            b->vparts = b->alloc<NlPick>((size_t)b->n_slots * D.max_tgt * kNlPickSlices);
            b->mapped(2 * kNlBatchMaxRows, &b->vres_host, &b->vres_dev);
        }
        for (int i = 0; i < n; ++i) b->vres_host[2 * i] = -1;
        nlb_prompt_upload(b, table);
        nlb_prefill_chain(b, total);
        // read-out: row 0 of a slot predicts the forced token and is projected with the rest (skipping it would cost a gather)
        const LaunchCtx c = b->ctx();
        for (int r0 = 0; r0 < total; r0 += kNlVerifyChunk) {
            const int rows = std::min(kNlVerifyChunk, total - r0);
            const size_t at = (size_t)r0 * D.d_model;
            nl_logits(c, b->m, /*fused=*/false, b->pws.x + at, rows, 1, b->pws.h + at, b->vlogits);
            launch_nllb_verify_pick_rows(c, b->vlogits, D.vocab, rows, b->vparts + (size_t)r0 * kNlPickSlices);
        }
        {
            KernelScope ks(c, "nllb_verify_accept");
            hipLaunchKernelGGL(nllb_verify_accept_kernel, dim3(n), dim3(64), 0, b->stream, b->vparts, b->prefill_rows, sl, b->vres_dev);
            WLK_HIP(hipGetLastError());
        }
        WLK_HIP(hipStreamSynchronize(b->stream));
        for (int i = 0; i < n; ++i)          // (before any slot changes)
            if (b->vres_host[2 * i] < 0 || b->vres_host[2 * i] > sl.P[i] - 2)
                throw std::runtime_error("NLLB batch verify: the accept kernel left no result");
        b->verify_passes += 1;
        for (int i = 0; i < n; ++i) {
            const int k = b->vres_host[2 * i];
            accepted[i] = k;
            next_token[i] = b->vres_host[2 * i + 1];
            NlBatchSlot& s = b->slots[slots[i]];
            s.self_len = 2 + k;              // the rows behind it hold the rejected draft: a step at o reads below o and writes o
            s.logits_row = -1;
            s.align_row = -1;
            b->verify_draft += (uint64_t)(sl.P[i] - 2);
            b->verify_accepted += (uint64_t)k;
        }
        return WLK_OK;
    });
}

int wlk_nllb_batch_verify_stats(wlk_nllb_batch* b, uint64_t* passes, uint64_t* draft_tokens, uint64_t* accepted_tokens) {
    if (!b || !passes || !draft_tokens || !accepted_tokens) return nl_fail(WLK_ERR_ARG, "NULL argument");
    *passes = b->verify_passes;
    *draft_tokens = b->verify_draft;
    *accepted_tokens = b->verify_accepted;
    return WLK_OK;
}

int wlk_nllb_batch_release(wlk_nllb_batch* b, int32_t slot) {
    if (!b) return nl_fail(WLK_ERR_ARG, "NULL argument");
    if (slot < 0 || slot >= b->n_slots) return nl_fail(WLK_ERR_ARG, "NLLB batch: slot index out of range");
    NlBatchSlot& s = b->slots[slot];
    s.encoded = false;
    s.src_len = s.self_len = 0;
    s.logits_row = -1;
    s.align_row = -1;
    return WLK_OK;
}

int wlk_nllb_batch_export(wlk_nllb_batch* b, int32_t slot, const char* what, float* host, uint64_t capacity, uint64_t* n_written) {
    if (!b || !what || !host || !n_written) return nl_fail(WLK_ERR_ARG, "NULL argument");
    if (slot < 0 || slot >= b->n_slots) return nl_fail(WLK_ERR_ARG, "NLLB batch: slot index out of range");
    return nl_guarded([&]() {
        const wlk_nllb_dims& D = b->m->D;
        const NlBatchSlot& s = b->slots[slot];
        const std::string w = what;
        const float* src = nullptr;
        uint64_t n = 0;
        if (!s.encoded) return nl_fail(WLK_ERR_STATE, "slot not encoded");
        if (w == "logits") {
            if (s.logits_row < 0) return nl_fail(WLK_ERR_STATE, "the slot was not in the latest step: no logits");
            src = b->logits + (size_t)s.logits_row * D.vocab; n = (uint64_t)D.vocab;
        } else if (w == "enc") {
            src = s.enc_out; n = (uint64_t)s.src_len * D.d_model;
        } else if (w == "align") {
            if (s.align_row < 0) return nl_fail(WLK_ERR_STATE, "the slot was not in the latest align step: no alignment");
            src = b->align_p + (size_t)s.align_row * D.max_src; n = (uint64_t)s.src_len;
        } else {
            return nl_fail(WLK_ERR_ARG, "unknown export " + w);
        }
        if (n > capacity) return nl_fail(WLK_ERR_CAPACITY, "export buffer too small");
        WLK_HIP(hipSetDevice(b->m->device));
        WLK_HIP(hipMemcpyAsync(host, src, n * sizeof(float), hipMemcpyDeviceToHost, b->stream));
        WLK_HIP(hipStreamSynchronize(b->stream));
        *n_written = n;
        return WLK_OK;
    });
}

int wlk_nllb_batch_cross_attention(wlk_nllb_batch* b, const int32_t* slots, int32_t n_rows, int32_t layer, const float* q_host,
                                   float* out_host) {
    if (!b || !slots || !q_host || !out_host) return nl_fail(WLK_ERR_ARG, "NULL argument");
    if (n_rows < 1 || n_rows > kNlBatchMaxRows || n_rows > b->n_slots) return nl_fail(WLK_ERR_ARG, "NLLB batch: 1..min(8, n_slots) rows");
    if (int rc = nlb_check_slots(b, slots, n_rows)) return rc;
    const wlk_nllb_dims& D = b->m->D;
    if (layer < 0 || layer >= D.dec_layers) return nl_fail(WLK_ERR_ARG, "decoder layer out of range");
    for (int r = 0; r < n_rows; ++r)
        if (!b->slots[slots[r]].encoded) return nl_fail(WLK_ERR_STATE, "NLLB batch: slot not encoded");
    return nl_guarded([&]() {
        const size_t d = D.d_model;
        StepRow table[kNlBatchMaxRows] = {};
        for (int r = 0; r < n_rows; ++r) table[r] = nlb_row(b, slots[r], 0);
        WLK_HIP(hipSetDevice(b->m->device));
        WLK_HIP(hipStreamSynchronize(b->stream));
        WLK_HIP(hipMemcpyAsync(b->probe_rows_dev, table, (size_t)n_rows * sizeof(StepRow), hipMemcpyHostToDevice, b->stream));
        WLK_HIP(hipMemcpyAsync(b->ws.q, q_host, (size_t)n_rows * d * sizeof(float), hipMemcpyHostToDevice, b->stream));
        WLK_HIP(hipStreamSynchronize(b->stream));           // `table` and q_host are pageable
        launch_nllb_cross_attention_ragged(b->ctx(), b->ws.q, b->probe_rows_dev, (long)layer * 2 * d, (long)D.dec_layers * 2 * d, b->ws.att,
                                           n_rows, (int)d, D.heads);
        WLK_HIP(hipMemcpyAsync(out_host, b->ws.att, (size_t)n_rows * d * sizeof(float), hipMemcpyDeviceToHost, b->stream));
        WLK_HIP(hipStreamSynchronize(b->stream));
        return WLK_OK;
    });
}

/* The ragged cross-attention on host data through its launchers, unchanged (see include/wlk_hip.h): a StepRow table whose
 * cross_kv / content_len are the caller's blocks and lengths.  Refusals (nllb_cross_ragged_check on the host's lengths and
 * ranks, and what a buffer cannot hold) come before anything is uploaded. */
int wlk_diag_nllb_cross_ragged(const wlk_diag_nllb_cross_ragged_args* g) {
    try {
        auto need = [](bool ok, const char* what) {
            if (!ok) throw std::invalid_argument(std::string("wlk_diag_nllb_cross_ragged: ") + what);
        };
        need(g != nullptr, "null arguments");
        need(g->q && g->kv && g->out && g->lengths && g->kv_at && g->kv_rows, "null q, kv, out, lengths, kv_at or kv_rows");
        const bool align = g->align != 0;
        need(g->n_rows >= 1 && g->n_rows <= 64 && g->n_head >= 1 && g->n_head <= 64 && g->d >= 1 && g->d <= 4096, "n_rows and n_head in [1, 64], d in [1, 4096]");
        need(g->ldkv >= 1 && g->ldkv <= (1 << 20) && g->kv_off >= 0 && g->kv_off <= (1 << 20), "ldkv in [1, 2^20], kv_off in [0, 2^20]");
        need(!align || (g->head_rank && g->align_probs && g->n_rank >= 1 && g->n_rank <= 64), "the align form needs head_rank, align_probs and 1 .. 64 ranks");
        nllb_cross_ragged_check(g->n_rows, g->d, g->n_head, (long)g->kv_off, (long)g->ldkv, g->lengths, align, g->head_rank, g->n_rank,
                                g->align_stride);
        const int64_t d = g->d;
        need((int64_t)g->n_rows * d <= g->q_floats && (int64_t)g->n_rows * d <= g->out_floats, "q / out hold fewer than n_rows x d floats");
        for (int r = 0; r < g->n_rows; ++r) {
            need(g->kv_rows[r] >= g->lengths[r], "a K/V block holds fewer rows than the row's length");
            need(g->kv_at[r] >= 0 && g->kv_at[r] % 4 == 0 && g->kv_at[r] + (int64_t)g->kv_rows[r] * g->ldkv <= g->kv_floats,
                 "a K/V block lies past kv (offsets are multiples of 4)");
        }
        need(!align || (int64_t)g->n_rank * kNlBatchMaxRows * g->align_stride <= g->probs_floats, "align_probs holds fewer than n_rank x 8 x align_stride floats");
        DevBytes Q, KV, OUT, PROBS, RANK;
        Q.mirror(g->q, (size_t)g->q_floats * 4);
        KV.mirror(g->kv, (size_t)g->kv_floats * 4);
        OUT.mirror(g->out, (size_t)g->out_floats * 4);
        if (align) {
            PROBS.mirror(g->align_probs, (size_t)g->probs_floats * 4);
            RANK.alloc((size_t)g->n_head * 4, g->head_rank);
        }
        std::vector<StepRow> table((size_t)g->n_rows);
        for (int r = 0; r < g->n_rows; ++r) {
            table[r] = StepRow{};
            table[r].cross_kv = KV.f() + g->kv_at[r];
            table[r].content_len = g->lengths[r];
        }
        DevBytes ROWS(table.size() * sizeof(StepRow), table.data());
        LaunchCtx ctx;
        WLK_HIP(hipDeviceSynchronize());
        const StepRow* rows = ROWS.as<const StepRow>();
        if (align)
            launch_nllb_cross_attention_ragged_align(ctx, Q.f(), rows, (long)g->kv_off, (long)g->ldkv, OUT.f(), g->n_rows, g->d, g->n_head,
                                                     RANK.i(), PROBS.f(), g->align_stride);
        else
            launch_nllb_cross_attention_ragged(ctx, Q.f(), rows, (long)g->kv_off, (long)g->ldkv, OUT.f(), g->n_rows, g->d, g->n_head);
        WLK_HIP(hipDeviceSynchronize());
        Q.back(); KV.back(); OUT.back(); PROBS.back();
        return WLK_OK;
    } catch (const std::invalid_argument& e) {      // nothing was uploaded or launched
        set_diag_error(e.what());
        return WLK_ERR_ARG;
    } catch (const std::exception& e) {
        set_diag_error(e.what());
        return WLK_ERR_HIP;
    }
}

int wlk_nllb_batch_sync(wlk_nllb_batch* b) {
    if (!b) return nl_fail(WLK_ERR_ARG, "NULL argument");
    return nl_guarded([&]() {
        WLK_HIP(hipSetDevice(b->m->device));
        WLK_HIP(hipStreamSynchronize(b->stream));
        return WLK_OK;
    });
}

}  // extern "C"
