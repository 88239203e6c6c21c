// CIF end-of-word head on the device (opt-in): what simul_whisper/eow_detection.py:37-77 computes from the
// content rows of the encoder output - alpha = sigmoid(Linear(d, 1)(x)), the `resize` rescaling, the integrate-and-fire
// test over the last two frames - as two small kernels behind the encoder, with the decision left in a host-coherent
// record that the caller reads when the policy finally asks for it (after the decode loop).  gfx950 only.
//
//   cif_alpha_kernel   one wave per encoder row, fp32 rows or the X3 image (x3.h) read directly
//   cif_decide_kernel  one workgroup per session over alpha[0, T): sum, rescale, resize loop, scan, fire test
//
// Every reduction has one fixed order that depends on neither T nor the grid nor the sessions stacked beside this one, so
// a session's alphas and record have the same bits alone and in a stacked encode.
#include <climits>
#include <cstring>

#include "internal.h"
#include "wave_ops.h"
#include "x3.h"

namespace wlk {
namespace {

constexpr int kCifChunks = 3;                      // 8-element chunks per lane: 64 lanes x 3 x 8 = 1536 >= kCifMaxD
constexpr int kCifMaxD = 1280;
constexpr int kCifWaves = 4, kCifRowsPerWave = 2;  // 8 rows per workgroup: 188 workgroups for 1500 rows
constexpr int kCifRun = 6;                         // contiguous alphas per thread of the decide kernel
constexpr int kCifMaxT = 256 * kCifRun;            // 1536 >= n_audio_ctx
constexpr float kCifThreshold = 0.999f;

struct CifArgs {
    const void* enc[kMaxBatch];     // [T][d] fp32, or the X3 image [T][3 d] bf16
    float* alpha[kMaxBatch];        // [T]
    wlk_cif_out* rec[kMaxBatch];    // host-coherent result record (device-side address)
    int T[kMaxBatch];               // content rows of session z (< 2: nothing to do)
    unsigned seq[kMaxBatch];
    const float* w;
    float bias;
    int d;
};

typedef const __attribute__((address_space(1))) x3_u32x4* gcu4_ptr;

__device__ __forceinline__ void pin_loaded_u4(x3_u32x4& a) { asm volatile("" : "+v"(a.x), "+v"(a.y), "+v"(a.z), "+v"(a.w)); }
__device__ __forceinline__ float bf16_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf16_hi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }

// Lane l owns the 8-element chunks l, l + 64, l + 128 of a row - a chunk is what one X3 triple of 16-byte units holds, so
// the fp32 and the X3 form give every lane the same values in the same order: fmaf chain over the lane's elements, then
// wave_sum.  All loads of the wave's rows (and of w) are issued before the first wait; chunks past d read chunk 0 and are
// replaced by zeros.
template <bool X3>
__global__ __launch_bounds__(256) void cif_alpha_kernel(CifArgs a) {
    const unsigned z = blockIdx.y;
    const int T = table_at(a.T, z);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row0 = ((int)blockIdx.x * kCifWaves + wave) * kCifRowsPerWave;
    if (row0 >= T) return;
    const int d = a.d, n_chunk = d >> 3;
    const void* enc = table_at(a.enc, z);
    float* alpha = table_at(a.alpha, z);

    bool ok[kCifChunks];
    int cc[kCifChunks];
#pragma unroll
    for (int j = 0; j < kCifChunks; ++j) {
        const int c = lane + 64 * j;
        ok[j] = c < n_chunk;
        cc[j] = ok[j] ? c : 0;
    }
    float4 w0[kCifChunks], w1[kCifChunks];
#pragma unroll
    for (int j = 0; j < kCifChunks; ++j) {
        const gcf_ptr wp = to_global(a.w) + cc[j] * 8;
        w0[j] = ldg4(wp);
        w1[j] = ldg4(wp + 4);
    }
    int rows[kCifRowsPerWave];
#pragma unroll
    for (int r = 0; r < kCifRowsPerWave; ++r) rows[r] = row0 + r < T ? row0 + r : row0;
    float x[kCifRowsPerWave][kCifChunks][8];
    if constexpr (X3) {
        x3_u32x4 u[kCifRowsPerWave][kCifChunks][3];
#pragma unroll
        for (int r = 0; r < kCifRowsPerWave; ++r)
#pragma unroll
            for (int j = 0; j < kCifChunks; ++j) {
                const gcu4_ptr p = (gcu4_ptr)enc + ((long)rows[r] * n_chunk + cc[j]) * 3;
                u[r][j][0] = p[0];
                u[r][j][1] = p[1];
                u[r][j][2] = p[2];
            }
#pragma unroll
        for (int r = 0; r < kCifRowsPerWave; ++r)
#pragma unroll
            for (int j = 0; j < kCifChunks; ++j) {
                pin_loaded_u4(u[r][j][0]);
                pin_loaded_u4(u[r][j][1]);
                pin_loaded_u4(u[r][j][2]);
            }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int r = 0; r < kCifRowsPerWave; ++r)
#pragma unroll
            for (int j = 0; j < kCifChunks; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i) {      // (hi + mid) + lo is the fp32 value the planes were split from, exactly
                    const unsigned h = u[r][j][0][i], m = u[r][j][1][i], l = u[r][j][2][i];
                    x[r][j][2 * i] = (bf16_lo(h) + bf16_lo(m)) + bf16_lo(l);
                    x[r][j][2 * i + 1] = (bf16_hi(h) + bf16_hi(m)) + bf16_hi(l);
                }
    } else {
        float4 v[kCifRowsPerWave][kCifChunks][2];
#pragma unroll
        for (int r = 0; r < kCifRowsPerWave; ++r)
#pragma unroll
            for (int j = 0; j < kCifChunks; ++j) {
                const gcf_ptr p = to_global(static_cast<const float*>(enc)) + (long)rows[r] * d + cc[j] * 8;
                v[r][j][0] = ldg4(p);
                v[r][j][1] = ldg4(p + 4);
            }
#pragma unroll
        for (int r = 0; r < kCifRowsPerWave; ++r)
#pragma unroll
            for (int j = 0; j < kCifChunks; ++j) {
                pin_loaded(v[r][j][0]);
                pin_loaded(v[r][j][1]);
            }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int r = 0; r < kCifRowsPerWave; ++r)
#pragma unroll
            for (int j = 0; j < kCifChunks; ++j) {
                x[r][j][0] = v[r][j][0].x; x[r][j][1] = v[r][j][0].y; x[r][j][2] = v[r][j][0].z; x[r][j][3] = v[r][j][0].w;
                x[r][j][4] = v[r][j][1].x; x[r][j][5] = v[r][j][1].y; x[r][j][6] = v[r][j][1].z; x[r][j][7] = v[r][j][1].w;
            }
    }
#pragma unroll
    for (int r = 0; r < kCifRowsPerWave; ++r) {
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < kCifChunks; ++j) {
            const float wv[8] = {w0[j].x, w0[j].y, w0[j].z, w0[j].w, w1[j].x, w1[j].y, w1[j].z, w1[j].w};
#pragma unroll
            for (int e = 0; e < 8; ++e) acc = fmaf(ok[j] ? x[r][j][e] : 0.f, ok[j] ? wv[e] : 0.f, acc);
        }
        const float zv = wave_sum(acc) + a.bias;
        const float al = 1.0f / (1.0f + expf(-zv));
        if (lane == 0 && row0 + r < T) alpha[row0 + r] = al;
    }
}

// ---- the decision ---------------------------------------------------------------------------------------------------
// Block-wide reductions over 256 threads: wave fold, four wave results through LDS, added in wave order.  The slots
// alternate so that one barrier per reduction is enough (a slot is rewritten only after the barrier of the next one).
struct CifShared {
    float sum[2][4], cnt[2][4], cur[2];
    int imin[4];
    int wtot[4];
    float ftot[4];
    float last;
    unsigned short cand[kCifMaxT];
};

__device__ __forceinline__ int wave_scan_incl(int v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(v, off, 64);
        if (lane >= off) v += o;
    }
    return v;
}
__device__ __forceinline__ float wave_scan_incl(float v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const float o = __shfl_up(v, off, 64);
        if (lane >= off) v += o;
    }
    return v;
}

// torch's floor division of fp32 values (c10::div_floor_floating): what `integrate[-1] // threshold` evaluates
__device__ __forceinline__ float div_floor_f32(float a, float b) {
    const float mod = fmodf(a, b);
    float div = (a - mod) / b;
    if (mod != 0.f && ((b < 0.f) != (mod < 0.f))) div -= 1.f;
    if (div != 0.f) {
        float fl = floorf(div);
        if (div - fl > 0.5f) fl += 1.f;
        return fl;
    }
    return copysignf(0.f, a / b);
}

__global__ __launch_bounds__(256) void cif_decide_kernel(CifArgs a) {
    __shared__ CifShared sh;
    const unsigned z = blockIdx.x;
    const int T = table_at(a.T, z);
    if (T < 2) return;
    const gcf_ptr alpha = to_global(table_at(a.alpha, z));
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int base = tid * kCifRun;
    int phase = 0;

    float v[kCifRun];
    bool valid[kCifRun];
#pragma unroll
    for (int e = 0; e < kCifRun; ++e) {
        valid[e] = base + e < T;
        v[e] = alpha[valid[e] ? base + e : 0];
    }
    // total = sum(alpha); n = round half to even; a = alpha * (n / total)
    float part = 0.f;
#pragma unroll
    for (int e = 0; e < kCifRun; ++e) part += valid[e] ? v[e] : 0.f;
    part = wave_sum(part);
    if (lane == 0) sh.sum[phase][wave] = part;
    __syncthreads();
    const float total = ((sh.sum[phase][0] + sh.sum[phase][1]) + sh.sum[phase][2]) + sh.sum[phase][3];
    phase ^= 1;
    const float n = rintf(total);
    const float scale = n / total;
    float av[kCifRun];
#pragma unroll
    for (int e = 0; e < kCifRun; ++e) av[e] = valid[e] ? v[e] * scale : 0.f;

    // resize (eow_detection.py:47-58): at most 10 rounds; a round visits, in index order, the elements that exceeded the
    // threshold when it began, and every one still at or above it halves the row towards its mean
    int rounds = 0;
    for (;;) {
        unsigned mask = 0;
#pragma unroll
        for (int e = 0; e < kCifRun; ++e) mask |= (valid[e] && av[e] > kCifThreshold) ? (1u << e) : 0u;
        const int mine = __popc(mask);
        const int incl = wave_scan_incl(mine, lane);
        if (lane == 63) sh.wtot[wave] = incl;
        __syncthreads();
        int off = incl - mine;
        for (int w = 0; w < wave; ++w) off += sh.wtot[w];
        const int n_cand = sh.wtot[0] + sh.wtot[1] + sh.wtot[2] + sh.wtot[3];
        if (n_cand == 0) break;          // (every thread sees the same count)
        if (rounds == 10) break;
        ++rounds;
#pragma unroll
        for (int e = 0; e < kCifRun; ++e)
            if (mask & (1u << e)) sh.cand[off++] = (unsigned short)(base + e);
        __syncthreads();
        for (int k = 0; k < n_cand; ++k) {
            const int idx = sh.cand[k];
            float s = 0.f, c = 0.f;
#pragma unroll
            for (int e = 0; e < kCifRun; ++e) {
                s += av[e];                                          // (rows past T hold zeros)
                c += (valid[e] && av[e] != 0.f) ? 1.f : 0.f;
            }
            s = wave_sum(s);
            c = wave_sum(c);
            if (lane == 0) {
                sh.sum[phase][wave] = s;
                sh.cnt[phase][wave] = c;
            }
            if (idx / kCifRun == tid) {
                float cur = av[0];
#pragma unroll
                for (int e = 1; e < kCifRun; ++e) cur = (idx - base == e) ? av[e] : cur;
                sh.cur[phase] = cur;
            }
            __syncthreads();
            if (sh.cur[phase] >= kCifThreshold) {
                const float S = ((sh.sum[phase][0] + sh.sum[phase][1]) + sh.sum[phase][2]) + sh.sum[phase][3];
                const float Cn = ((sh.cnt[phase][0] + sh.cnt[phase][1]) + sh.cnt[phase][2]) + sh.cnt[phase][3];
                const float mean = 0.5f * S / Cn;
#pragma unroll
                for (int e = 0; e < kCifRun; ++e)
                    if (valid[e]) av[e] = av[e] * 0.5f + mean * (av[e] != 0.f ? 1.f : 0.f);
            }
            phase ^= 1;
        }
        __syncthreads();                 // the candidate list and wtot are rewritten by the next round
    }
    __syncthreads();                     // wtot was read above; ftot / imin below are separate, this orders the exit paths

    // integ = inclusive scan of a[0 .. T-1); the last frame is left out (eow_detection.py:70)
    float loc[kCifRun];
    float run = 0.f;
#pragma unroll
    for (int e = 0; e < kCifRun; ++e) {
        run += (base + e < T - 1) ? av[e] : 0.f;
        loc[e] = run;
    }
    const float fincl = wave_scan_incl(run, lane);
    float fexcl = __shfl_up(fincl, 1, 64);
    if (lane == 0) fexcl = 0.f;
    if (lane == 63) sh.ftot[wave] = fincl;
    __syncthreads();
    float woff = 0.f;
    for (int w = 0; w < wave; ++w) woff += sh.ftot[w];
    const float before = woff + fexcl;
    float integ[kCifRun];
#pragma unroll
    for (int e = 0; e < kCifRun; ++e) integ[e] = before + loc[e];
    if ((T - 2) / kCifRun == tid) {
        float last = integ[0];
#pragma unroll
        for (int e = 1; e < kCifRun; ++e) last = ((T - 2) - base == e) ? integ[e] : last;
        sh.last = last;
    }
    __syncthreads();
    const float integ_last = sh.last;
    const float cntf = div_floor_f32(integ_last, kCifThreshold);
    int first = INT_MAX;
#pragma unroll
    for (int e = kCifRun - 1; e >= 0; --e)
        if (base + e < T - 1 && integ[e] - cntf * 1.0f >= 0.f) first = base + e;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) first = min(first, __shfl_xor(first, off, 64));
    if (lane == 0) sh.imin[wave] = first;
    __syncthreads();
    if (tid == 0) {
        const int pos = min(min(sh.imin[0], sh.imin[1]), min(sh.imin[2], sh.imin[3]));
        wlk_cif_out* rec = table_at(a.rec, z);
        rec->fire = (pos != INT_MAX && pos >= T - 2) ? 1 : 0;
        rec->n = (n == n && fabsf(n) < 1e9f) ? (int)n : -1;
        rec->cnt = (cntf == cntf && fabsf(cntf) < 1e9f) ? (int)cntf : -1;
        rec->pos = pos == INT_MAX ? -1 : pos;
        rec->resize_rounds = rounds;
        rec->total = total;
        rec->integ_last = integ_last;
        __threadfence_system();          // the fields are visible to the host before the sequence number is
        *(volatile uint32_t*)&rec->seq = table_at(a.seq, z);
    }
}

void launch_cif(const LaunchCtx& c, const CifArgs& a, int n, int max_T, bool x3) {
    if (n < 1 || max_T < 2) return;
    {
        KernelScope k(c, "cif_alpha", 2.0 * n * max_T * a.d, (double)n * max_T * a.d * (x3 ? 6.0 : 4.0));
        const dim3 grid((max_T + kCifWaves * kCifRowsPerWave - 1) / (kCifWaves * kCifRowsPerWave), n);
        if (x3) hipLaunchKernelGGL(cif_alpha_kernel<true>, grid, dim3(256), 0, c.stream, a);
        else hipLaunchKernelGGL(cif_alpha_kernel<false>, grid, dim3(256), 0, c.stream, a);
        WLK_HIP(hipGetLastError());
    }
    {
        KernelScope k(c, "cif_decide", 0.0, (double)n * max_T * 4.0);
        hipLaunchKernelGGL(cif_decide_kernel, dim3(n), dim3(256), 0, c.stream, a);
        WLK_HIP(hipGetLastError());
    }
}

bool cif_shape_ok(int d, int n_ctx) { return d >= 8 && d % 8 == 0 && d <= kCifMaxD && n_ctx >= 1 && n_ctx <= kCifMaxT; }

// host-coherent record block: written by the decide kernel with plain stores, read by the host without a copy
void cif_record_alloc(wlk_cif_out** host, wlk_cif_out** dev, int n) {
    void *hp = nullptr, *dp = nullptr;
    WLK_HIP(hipHostMalloc(&hp, (size_t)n * sizeof(wlk_cif_out), hipHostMallocMapped | hipHostMallocCoherent));
    std::memset(hp, 0, (size_t)n * sizeof(wlk_cif_out));
    if (hipError_t e = hipHostGetDevicePointer(&dp, hp, 0); e != hipSuccess) {
        (void)hipHostFree(hp);
        WLK_HIP(e);
    }
    *host = static_cast<wlk_cif_out*>(hp);
    *dev = static_cast<wlk_cif_out*>(dp);
}

}  // namespace
}  // namespace wlk

using namespace wlk;

// The session's share of the feature: the alpha row and the record block.  Called at session creation when the model
// already has a head, otherwise by the first encode that finds one.
void wlk_cif_session_prepare(wlk_session* s) {
    if (s->cif_host) return;
    s->cif_alpha = dev_alloc<float>(s->m->D.n_audio_ctx);
    cif_record_alloc(&s->cif_host, &s->cif_host_dev, 1);
}

void wlk_cif_session_free(wlk_session* s) {
    if (s->cif_alpha) (void)hipFree(s->cif_alpha);
    if (s->cif_host) (void)hipHostFree(s->cif_host);
    s->cif_alpha = nullptr;
    s->cif_host = s->cif_host_dev = nullptr;
}

// Behind the cross-K/V GEMM of an encode chain (wlk_encode_group), on the chain's stream: both kernels for every session
// of the group whose content is at least two frames.
void wlk_cif_enqueue(const std::vector<wlk_session*>& group, const LaunchCtx& c, const std::vector<int>& content) {
    wlk_model* m = group[0]->m;
    const bool x3 = m->xkv_all_w3 != nullptr;
    CifArgs a{};
    a.w = m->cif_w;
    a.bias = m->cif_b;
    a.d = m->D.n_audio_state;
    int max_T = 0;
    for (size_t i = 0; i < group.size(); ++i) {
        wlk_session* s = group[i];
        wlk_cif_session_prepare(s);
        const int T = std::max(0, std::min(content[i], (int)m->D.n_audio_ctx));
        s->cif_T = T;
        s->cif_stream = c.stream;
        s->cif_seq += 1;
        if (s->cif_seq == 0) s->cif_seq = 1;       // 0 is the freshly zeroed record
        a.enc[i] = x3 ? static_cast<const void*>(s->enc_out3) : static_cast<const void*>(s->enc_out);
        a.alpha[i] = s->cif_alpha;
        a.rec[i] = s->cif_host_dev;
        a.T[i] = T >= 2 ? T : 0;
        a.seq[i] = s->cif_seq;
        max_T = std::max(max_T, a.T[i]);
    }
    launch_cif(c, a, (int)group.size(), max_T, x3);
}

extern "C" {

int wlk_model_set_cif(wlk_model* m, const float* weight_host, int d, float bias) {
    if (!m) return fail(WLK_ERR_ARG, "model is NULL");
    if (!m->finalized) return fail(WLK_ERR_STATE, "model not finalized");
    if (weight_host && d != m->D.n_audio_state) return fail(WLK_ERR_ARG, "CIF head: d must equal n_audio_state");
    if (weight_host && !cif_shape_ok(d, m->D.n_audio_ctx))
        return fail(WLK_ERR_ARG, "CIF head: the device kernels take d % 8 == 0, d <= 1280 and n_audio_ctx <= 1536");
    return guarded([&]() {
        WLK_HIP(hipSetDevice(m->device));
        // not to be called while an encode of this model is in flight (the Python layer sets the head once, under the
        // model's lock, before the first session encodes)
        WLK_HIP(hipDeviceSynchronize());
        if (m->cif_w) (void)hipFree(m->cif_w);
        m->cif_w = nullptr;
        m->cif_b = 0.f;
        if (weight_host) {
            float* w = dev_alloc<float>(d);
            try {
                copy_sync(w, weight_host, (size_t)d * sizeof(float), hipMemcpyHostToDevice);
            } catch (...) {
                (void)hipFree(w);
                throw;
            }
            m->cif_w = w;
            m->cif_b = bias;
        }
        return WLK_OK;
    });
}

int wlk_cif_result(wlk_session* s, wlk_cif_out* out) {
    if (!s || !out) return fail(WLK_ERR_ARG, "NULL argument");
    if (!s->m->cif_w) return fail(WLK_ERR_STATE, "the model has no CIF head");
    if (s->cif_T < 0 || !s->cif_host) return fail(WLK_ERR_STATE, "nothing has been encoded with the CIF head");
    if (s->cif_T < 2) return fail(WLK_ERR_STATE, "CIF: the last encode had fewer than two content frames");
    return guarded([&]() {
        const volatile wlk_cif_out* rec = s->cif_host;
        if (__atomic_load_n(&s->cif_host->seq, __ATOMIC_ACQUIRE) != s->cif_seq) {
            // the kernels are still queued or running: wait for the stream the encode ran on (a stacked encode has been
            // waited for by the engine already), then look once more - no spinning
            WLK_HIP(hipSetDevice(s->m->device));
            WLK_HIP(hipStreamSynchronize(s->cif_stream));
            if (__atomic_load_n(&s->cif_host->seq, __ATOMIC_ACQUIRE) != s->cif_seq)
                throw std::runtime_error("CIF: the encode finished without delivering its record");
        }
        out->fire = rec->fire; out->n = rec->n; out->cnt = rec->cnt; out->pos = rec->pos;
        out->resize_rounds = rec->resize_rounds; out->total = rec->total; out->integ_last = rec->integ_last;
        out->seq = s->cif_seq;
        return WLK_OK;
    });
}

int wlk_diag_cif(const float* feat_host, int T, int d, const float* weight, float bias, int as_x3, int n_stack,
                 const int32_t* t_each, float* alphas_out, wlk_cif_out* out) {
    auto bad = [](const char* msg) {
        set_last_error(msg);
        return WLK_ERR_ARG;
    };
    if (!feat_host || !weight || !out) return bad("wlk_diag_cif: NULL argument");
    if (n_stack < 1 || n_stack > kMaxBatch) return bad("wlk_diag_cif: n_stack must be in [1, 8]");
    if (T < 1 || !cif_shape_ok(d, T)) return bad("wlk_diag_cif: needs 1 <= T <= 1536, d % 8 == 0, d <= 1280");
    for (int i = 0; t_each && i < n_stack; ++i)
        if (t_each[i] < 0 || t_each[i] > T) return bad("wlk_diag_cif: t_each out of [0, T]");
    float *feat = nullptr, *w = nullptr, *alpha = nullptr;
    unsigned short* feat3 = nullptr;
    wlk_cif_out *rec = nullptr, *rec_dev = nullptr;
    int rc = WLK_OK;
    try {
        const size_t per = (size_t)T * d;
        feat = dev_alloc<float>(per * n_stack);
        w = dev_alloc<float>(d);
        alpha = dev_alloc<float>((size_t)T * n_stack);
        WLK_HIP(hipMemcpy(feat, feat_host, per * n_stack * sizeof(float), hipMemcpyHostToDevice));
        WLK_HIP(hipMemcpy(w, weight, (size_t)d * sizeof(float), hipMemcpyHostToDevice));
        WLK_HIP(hipMemset(alpha, 0, (size_t)T * n_stack * sizeof(float)));
        cif_record_alloc(&rec, &rec_dev, n_stack);
        LaunchCtx c;
        if (as_x3) {
            feat3 = dev_alloc<unsigned short>(per * 3 * n_stack);
            launch_x3_pack(c, feat, d, feat3, d, T * n_stack, d);
        }
        CifArgs a{};
        a.w = w; a.bias = bias; a.d = d;
        int max_T = 0;
        for (int i = 0; i < n_stack; ++i) {
            const int Ti = t_each ? t_each[i] : T;
            a.enc[i] = as_x3 ? static_cast<const void*>(feat3 + per * 3 * i) : static_cast<const void*>(feat + per * i);
            a.alpha[i] = alpha + (size_t)T * i;
            a.rec[i] = rec_dev + i;
            a.T[i] = Ti >= 2 ? Ti : 0;
            a.seq[i] = 1;
            max_T = std::max(max_T, a.T[i]);
        }
        launch_cif(c, a, n_stack, max_T, as_x3 != 0);
        WLK_HIP(hipDeviceSynchronize());
        if (alphas_out) WLK_HIP(hipMemcpy(alphas_out, alpha, (size_t)T * n_stack * sizeof(float), hipMemcpyDeviceToHost));
        for (int i = 0; i < n_stack; ++i) {
            std::memcpy(&out[i], &rec[i], sizeof(wlk_cif_out));
            if (a.T[i] >= 2 && rec[i].seq != 1) throw std::runtime_error("wlk_diag_cif: no record was delivered");
        }
    } catch (const std::exception& e) {
        set_last_error(e.what());
        rc = WLK_ERR_HIP;
    }
    if (feat) (void)hipFree(feat);
    if (feat3) (void)hipFree(feat3);
    if (w) (void)hipFree(w);
    if (alpha) (void)hipFree(alpha);
    if (rec) (void)hipHostFree(rec);
    return rc;
}

}  // extern "C"
