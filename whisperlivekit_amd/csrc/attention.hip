// Encoder self-attention (whisper/model.py:148-173 with xa=None, mask=None): the reference
// materialises fp32 QK [H, 1500, 1500] per layer and throws it away (model.py:251); here the
// scores never leave registers.
//
// One 256-thread workgroup = one (head, 32-query tile).  Its four waves split the KEY axis:
// wave w takes key tiles w, w+4, w+8, ... (32 keys each) and keeps its own online-softmax state
// (running max m, running sum l, 64x32 output accumulator); the four partial states are merged
// through LDS at the end.  That gives 4 x 376 = 1504 independent MFMA streams for base.en
// (8 heads x 47 query tiles) - enough to cover the 1024 SIMDs of the chip, which 32-query tiles
// alone (376 waves) would not.
//
// Matrix core usage (v_mfma_f32_32x32x2_f32, exact fp32):
//   S^T[key][q]  = sum_d K[key][d] Q[q][d]          A = K tile, B = Q tile (both LDS, row stride 68:
//                                                    conflict-free ds_read_b128 of 4 consecutive d)
//   O^T[d][q]   += sum_key V[key][d] P^T[key][q]     A = V tile (LDS), B = P^T = the S^T accumulator
//                                                    registers themselves (C layout of step 1 is the
//                                                    B layout of step 2 up to a key permutation that the
//                                                    V fetch follows) - no shuffle, no LDS round trip.
// With S^T (keys on rows) every lane owns ONE query column, so the softmax row reductions are
// 15 in-lane ops + one cross-half swap, and the alpha rescale is a per-lane scalar.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>

#include "common.h"
#include "wave_ops.h"

namespace wlk {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int QT = 32, KT = 32, NWAVE = 4, K_LD = 68, O_LD = 65;
constexpr int kAttnLdsFloats = NWAVE * KT * K_LD + NWAVE * KT * 64;  // K tiles + V tiles
constexpr int kAttnLdsTotal = kAttnLdsFloats + QT * K_LD;            // + Q tile

// The decoder's PREFILL cross-attention (q rows = all fed tokens of all beams, k/v = the 1500 projected encoder
// positions).  Heads that are AlignAtt alignment heads also dump their raw scores into the session's alignment window
// (softmaxed in place afterwards by ring_softmax_kernel), so the [H, q, 1500] QK tensor of the reference is never
// formed for the other heads.  The encoder (q, k, v interleaved in one [T][3d] buffer) runs the same arithmetic in
// enc_attention_pw_kernel below.
__global__ __launch_bounds__(256) void flash_attention_kernel(FlashArgs a) {
    WLK_PIN_FLASH_ARGS(a);
    extern __shared__ __attribute__((aligned(16))) float lds[];
    // batched encodes: session blockIdx.y (locals: writing into `a` would put the argument struct into scratch memory)
    const bool batched = a.batch > 0;
    const float* const aq = batched ? table_at(a.z.in, blockIdx.y) : a.q;
    const float* const ak = batched ? aq + a.z_k_off : a.k;
    const float* const av = batched ? aq + a.z_v_off : a.v;
    float* const aout = batched ? table_at(a.z.out, blockIdx.y) : a.out;
    const int T = a.Tk;
    const int n_head = a.n_head;
    float* Ks = lds;                            // [NWAVE][KT][K_LD]
    float* Vs = lds + NWAVE * KT * K_LD;        // [NWAVE][KT][64]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int head = blockIdx.x % n_head;       // head == XCD for 8 heads: K/V of a head stay in one L2
    const int q_tiles = (a.Tq + QT - 1) / QT;
    const int qt_idx = (blockIdx.x / n_head) % q_tiles;
    const int ks = blockIdx.x / (n_head * q_tiles);   // key split index (0 when a.k_splits == 1)
    const int q0 = qt_idx * QT;
    const long ld = a.ldkv;
    const int half = lane >> 5;
    const int lq = lane & 31;


    f32x16 o0, o1;
#pragma unroll
    for (int i = 0; i < 16; ++i) { o0[i] = 0.f; o1[i] = 0.f; }
    float m_run = -INFINITY, l_run = 0.f;

    // staging map: per iteration 128 keys x 64 floats for K and for V = 2048 float4 each, 8 per thread
    // stacked prefills: this query tile's session supplies the keys / values and the alignment window
    // (round 4: global address space kept explicit - a pointer loaded from the tile table made these flat loads; no
    // select on the loaded VALUES - hipcc turned `ok ? k4 : 0` into one predicated branch per load with waits in between:
    // rows past T are fetched from row 0 instead, their scores are set to -inf below and their probabilities are 0)
    const gcf_ptr tk = to_global(a.tile_rows ? a.tile_rows[qt_idx].cross_kv + a.tile_kv_off : ak);
    const gcf_ptr kbase = tk + head * 64;
    const gcf_ptr vbase = (a.tile_rows ? tk + a.tile_v_off : to_global(av)) + head * 64;
    float4 rk[8], rv[8];
    auto fetch = [&](int it) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int idx = tid + 256 * i;
            const int key = it * (NWAVE * KT) + (idx >> 4);
            const int c4 = idx & 15;
            const long off = (long)(key < T ? key : 0) * ld + c4 * 4;
            rk[i] = ldg4(kbase + off);
            rv[i] = ldg4(vbase + off);
        }
    };
    // key range of this workgroup: iterations [it_lo, it_hi) of 128 keys each
    const int n_iter_all = (T + NWAVE * KT - 1) / (NWAVE * KT);
    const int it_per = (n_iter_all + a.k_splits - 1) / a.k_splits;
    const int it_lo = ks * it_per;
    const int n_iter = min(n_iter_all, it_lo + it_per);
    fetch(it_lo);     // in flight while the Q tile is staged and the alignment-head bookkeeping below resolves
    // alignment-window bookkeeping of this lane's query row: requested together with the tiles (each used to be its own
    // memory round trip in front of the first key tile)
    // (unconditional loads from pointers that are always readable - an absent table points at the queries - and pinned
    // behind the Q staging: a load inside a branch, or one hipcc can sink into one, costs its own wait)
    const int bk_row = min(q0 + lq, a.Tq - 1);
    const int* const any_ints = reinterpret_cast<const int*>(aq);
    int rank_raw = (a.head_rank ? a.head_rank + head : any_ints)[0];
    int ring_row_v = (a.ring_row ? a.ring_row + bk_row : any_ints)[0];
    int beam_v = (a.beam_of_row ? a.beam_of_row + bk_row : any_ints)[0];
    // Q tile -> LDS once ([32][K_LD], same padded layout as the K tiles); the B fragments are
    // re-read per key tile (one ds_read_b128 per 4 MFMAs - the 64-cycle fp32 MFMA leaves the LDS idle)
    float* Qs = lds + kAttnLdsFloats;
    static_assert(QT * 16 == 2 * 256, "two float4 of the Q tile per thread");
    {
        float4 qv[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int i = tid + 256 * j, qr = i >> 4, c4 = i & 15;
            qv[j] = *reinterpret_cast<const float4*>(aq + (long)min(q0 + qr, a.Tq - 1) * a.ldq + head * 64 + c4 * 4);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int i = tid + 256 * j, qr = i >> 4, c4 = i & 15;
            *reinterpret_cast<float4*>(&Qs[qr * K_LD + c4 * 4]) = q0 + qr < a.Tq ? qv[j] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    const float* Qw = Qs + lq * K_LD + half * 4;
    asm volatile("" : "+v"(rank_raw), "+v"(ring_row_v), "+v"(beam_v));
    const int rank = a.head_rank ? rank_raw : -1;
    // alignment-head score dump (decoder prefill only): pointer resolved from the values requested above
    float* dump = nullptr;
    if (rank >= 0 && q0 + lq < a.Tq) {
        if (a.tile_rows) dump = a.tile_rows[qt_idx].ring + ((long)rank * a.ring_rows + ring_row_v) * (long)T;
        else dump = a.ring + (((long)rank * a.n_beam + beam_v) * a.ring_rows + ring_row_v) * (long)T;
    }
    auto stash = [&]() {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int idx = tid + 256 * i;
            const int kl = idx >> 4;  // 0..127: tile = kl >> 5, row = kl & 31
            const int c4 = idx & 15;
            *reinterpret_cast<float4*>(&Ks[(kl >> 5) * (KT * K_LD) + (kl & 31) * K_LD + c4 * 4]) = rk[i];
            *reinterpret_cast<float4*>(&Vs[kl * 64 + c4 * 4]) = rv[i];
        }
    };

    const float* Kw = Ks + wave * (KT * K_LD) + lq * K_LD + half * 4;
    const float* Vw = Vs + wave * (KT * 64) + lq;

    for (int it = it_lo; it < n_iter; ++it) {
        __syncthreads();  // previous iteration's LDS reads are done
        stash();
        __syncthreads();
        if (it + 1 < n_iter) fetch(it + 1);

        const int key0 = it * (NWAVE * KT) + wave * KT;
        if (key0 < T) {  // wave-uniform
            f32x16 s;
#pragma unroll
            for (int i = 0; i < 16; ++i) s[i] = 0.f;
            // the 32 MFMAs are one dependent chain and the wave issues in order: the LDS fragments of group g+1 are
            // requested right after the first MFMA of group g has been issued (same idea as gemm_f32.hip)
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
            // rows of s: key = key0 + (r&3) + 8*(r>>2) + 4*half ; column: query lq
            if (dump) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int key = key0 + 8 * g + 4 * half;
                    if (key < T)   // T % 4 == 0 is checked by the launcher when dumping
                        *reinterpret_cast<float4*>(dump + key) = make_float4(s[4 * g], s[4 * g + 1], s[4 * g + 2], s[4 * g + 3]);
                }
            }
            float mt = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = key0 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (key >= T) s[r] = -INFINITY;
                mt = fmaxf(mt, s[r]);
            }
            mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
            const float m_new = fmaxf(m_run, mt);
            const float alpha = __expf(m_run - m_new);
            float rs = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                s[r] = __expf(s[r] - m_new);   // v_exp_f32: ~1 ulp, keeps the VALU share small next to the MFMAs
                rs += s[r];
            }
            rs += __shfl_xor(rs, 32, 64);
            l_run = l_run * alpha + rs;
            m_run = m_new;
#pragma unroll
            for (int i = 0; i < 16; ++i) { o0[i] *= alpha; o1[i] *= alpha; }
            // V values of key r+1 are requested before the two MFMAs of key r are issued (one LDS latency ahead)
            float v0 = Vw[(4 * half) * 64], v1 = Vw[(4 * half) * 64 + 32];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float v0n = v0, v1n = v1;
                if (r + 1 < 16) {
                    const int kn = ((r + 1) & 3) + 8 * ((r + 1) >> 2) + 4 * half;
                    v0n = Vw[kn * 64];
                    v1n = Vw[kn * 64 + 32];
                }
                __builtin_amdgcn_sched_barrier(0);
                o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(v0, s[r], o0, 0, 0, 0);
                o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(v1, s[r], o1, 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                v0 = v0n;
                v1 = v1n;
            }
        }
    }

    // merge the four key-split partial states through LDS (reusing the staging area)
    __syncthreads();
    float* Os = lds;                               // [NWAVE][QT][O_LD]
    float* Ms = lds + NWAVE * QT * O_LD;           // [NWAVE][QT]
    float* Ls = Ms + NWAVE * QT;                   // [NWAVE][QT]
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int dd = (r & 3) + 8 * (r >> 2) + 4 * half;
        Os[(wave * QT + lq) * O_LD + dd] = o0[r];
        Os[(wave * QT + lq) * O_LD + 32 + dd] = o1[r];
    }
    if (half == 0) {
        Ms[wave * QT + lq] = m_run;
        Ls[wave * QT + lq] = l_run;
    }
    __syncthreads();
    {
        const int dd = tid & 63;
        const int qg = tid >> 6;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int q = qg * 8 + i;
            const int qrow = q0 + q;
            float M = Ms[q];
#pragma unroll
            for (int w = 1; w < NWAVE; ++w) M = fmaxf(M, Ms[w * QT + q]);
            float L = 0.f, acc = 0.f;
#pragma unroll
            for (int w = 0; w < NWAVE; ++w) {
                const float e = expf(Ms[w * QT + q] - M);
                L += e * Ls[w * QT + q];
                acc += e * Os[(w * QT + q) * O_LD + dd];
            }
            if (a.k_splits == 1) {
                if (qrow < a.Tq) aout[(long)qrow * a.ldo + head * 64 + dd] = acc / L;
            } else if (qrow < a.Tq) {
                // partial state of this key range: unnormalised O (relative to M), M and L
                const long slot = ((long)qrow * n_head + head) * a.k_splits + ks;
                a.part_o[slot * 64 + dd] = acc;
                if (dd == 0) { a.part_m[slot] = M; a.part_l[slot] = L; }
            }
        }
    }
}


// ---------------------------------------------------------------------------------------------------------------------
// Encoder self-attention with wave-private staging ("pw"): the arithmetic of flash_attention_kernel - same (head,
// 32-query tile) workgroups, wave w takes key tiles w, w+4, ..., same MFMA sequences, same online-softmax updates,
// same four-way merge, so the output is bit-identical to it - but no workgroup barrier inside the key loop.
// flash_attention_kernel stages 128 keys per trip with all 256 threads (global -> registers -> LDS) between two
// __syncthreads(), although each wave only ever reads ITS OWN 32-key tile back: a third of the kernel's time was that
// staging (scripts/probes/attn_ablation.hip).  Here every wave fetches its own tiles by LDS-DMA into a private 16 KiB
// region - K(t) while the previous tile's P.V runs, V(t) while Q.K^T(t) runs - so the only waits are the wave's own
// s_waitcnt vmcnt(0) at the two phase changes, and the four waves of a workgroup drift freely.  The DMA writes
// lane-linearly; rows are 256 bytes, so the bank swizzle (16-byte chunk c of key row r stored at chunk c ^ (r & 15)) is
// applied to the source address and to the reads.  Fragment reads are inline asm: hipcc would drain the DMA queue in
// front of every LDS read that follows an LDS-DMA.  Q fragments live in registers.  64 KiB of LDS: two workgroups per
// CU, as before.
// ---------------------------------------------------------------------------------------------------------------------
typedef float f32x4a __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void enc_attention_pw_kernel(FlashArgs a) {
    WLK_PIN_FLASH_ARGS(a);
    extern __shared__ __attribute__((aligned(1024))) float lds[];
    const bool batched = a.batch > 0;
    const float* const aq = batched ? table_at(a.z.in, blockIdx.y) : a.q;
    const float* const ak = batched ? aq + a.z_k_off : a.k;
    const float* const av = batched ? aq + a.z_v_off : a.v;
    float* const aout = batched ? table_at(a.z.out, blockIdx.y) : a.out;
    const int T = a.Tk, n_head = a.n_head;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int head = blockIdx.x % n_head;       // head == XCD for 8 heads: K/V of a head stay in one L2
    const int qt_idx = blockIdx.x / n_head;
    const int q0 = qt_idx * QT;
    const long ld = a.ldkv;
    const int half = lane >> 5, lq = lane & 31;

    float4 qf[8];                               // Q[q0 + lq][8 g + 4 half .. +4]
    {
        const bool ok = q0 + lq < a.Tq;
        const float* qp = aq + (long)(ok ? q0 + lq : 0) * a.ldq + head * 64 + half * 4;
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            const float4 v = *reinterpret_cast<const float4*>(qp + g * 8);
            qf[g] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    f32x16 o0, o1;
#pragma unroll
    for (int i = 0; i < 16; ++i) { o0[i] = 0.f; o1[i] = 0.f; }
    float m_run = -INFINITY, l_run = 0.f;

    // private regions of this wave: K tile [32 keys][16 chunks of 16 bytes], V tile the same
    float* Kb = lds + wave * 4096;
    float* Vb = Kb + 2048;
    const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) float*)lds;
    const unsigned kb_addr = lds_base + (unsigned)wave * 16384u, vb_addr = kb_addr + 8192u;
    // DMA piece p (0..7) of a tile = key rows 4p .. 4p+3; lane l fills slot (row 4p + (l >> 4), chunk l & 15) with source
    // chunk (l & 15) ^ (row & 15)
    const int prow = lane >> 4;
    const float* kbase = ak + head * 64;
    const float* vbase = av + head * 64;
    auto dma_piece = [&](const float* base, float* dst, int key0, int p) {
        const int row = 4 * p + prow;
        const int chunk = (lane & 15) ^ (row & 15);
        const float* src = base + (long)min(key0 + row, T - 1) * ld + chunk * 4;   // rows past T: clamped, masked below
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)(dst + p * 256), 16, 0, 0);
    };
    // K fragment of group g: row lq, chunk 2g + half  ->  stored chunk (2g) ^ (half ^ (lq & 15))
    const unsigned k_row = kb_addr + (unsigned)lq * 256u;
    const unsigned k_h16 = (unsigned)(half ^ (lq & 15)) << 4;
    // V values of key kn = rs + 4 half (rs = (r & 3) + 8 (r >> 2)): d = lq and d = lq + 32
    const unsigned v_base = vb_addr + (unsigned)half * 1024u + (unsigned)(lq & 3) * 4u;
    const unsigned v_c0 = (unsigned)((lq >> 2) ^ (4 * half));
    auto v_addr = [&](int rs, int hi) { return v_base + (unsigned)rs * 256u + (((v_c0 ^ (unsigned)(hi * 8)) ^ (unsigned)(rs & 15)) << 4); };

    // the four streams of this workgroup: wave w takes key tiles w, w + 4, ...
    const int n_tiles = (T + KT - 1) / KT;
    const bool live = q0 < a.Tq;
    if (live && wave < n_tiles) {
#pragma unroll
        for (int p = 0; p < 8; ++p) dma_piece(kbase, Kb, wave * KT, p);
    }
    for (int t = wave; live && t < n_tiles; t += NWAVE) {
        const int key0 = t * KT;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // K(t) has landed (the only DMA this wave has in flight)
        // ---- S^T = K Q^T, with the eight pieces of V(t) dealt between the MFMAs
        f32x16 s;
#pragma unroll
        for (int i = 0; i < 16; ++i) s[i] = 0.f;
        f32x4a kc, kn;
        asm volatile("ds_read_b128 %0, %1" : "=v"(kc) : "v"(k_row + k_h16));
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(kc));
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            if (g + 1 < 8) asm volatile("ds_read_b128 %0, %1" : "=v"(kn) : "v"(k_row + (k_h16 ^ (unsigned)((g + 1) * 32))));
            __builtin_amdgcn_sched_barrier(0);
            s = __builtin_amdgcn_mfma_f32_32x32x2f32(kc[0], qf[g].x, s, 0, 0, 0);
            dma_piece(vbase, Vb, key0, g);
            s = __builtin_amdgcn_mfma_f32_32x32x2f32(kc[1], qf[g].y, s, 0, 0, 0);
            s = __builtin_amdgcn_mfma_f32_32x32x2f32(kc[2], qf[g].z, s, 0, 0, 0);
            s = __builtin_amdgcn_mfma_f32_32x32x2f32(kc[3], qf[g].w, s, 0, 0, 0);
            if (g + 1 < 8) {
                __builtin_amdgcn_sched_barrier(0);      // the wait stays BEHIND the group's MFMAs: they cover the read's latency
                asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(kn));
                kc = kn;
            }
        }
        // ---- online softmax (flash_attention_kernel's, verbatim)
        float mt = -INFINITY;
        if (key0 + KT > T) {        // only the last tile has keys past the end (wave-uniform)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = key0 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (key >= T) s[r] = -INFINITY;
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) mt = fmaxf(mt, s[r]);
        mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
        const float m_new = fmaxf(m_run, mt);
        const float alpha = __expf(m_run - m_new);
        float rs = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            s[r] = __expf(s[r] - m_new);
            rs += s[r];
        }
        rs += __shfl_xor(rs, 32, 64);
        l_run = l_run * alpha + rs;
        m_run = m_new;
        // once the running maxima have settled alpha is exactly 1.0f in every lane and the rescale (32 multiplies through
        // the accumulator file) is the identity: skipped then, bit for bit the same result
        if (__builtin_amdgcn_ballot_w64(alpha != 1.0f) != 0) {
#pragma unroll
            for (int i = 0; i < 16; ++i) { o0[i] *= alpha; o1[i] *= alpha; }
        }
        // ---- O^T += V P^T, with the eight pieces of K(t + 4) dealt between the MFMAs
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // V(t) has landed
        const bool more = t + NWAVE < n_tiles;
        float v0, v1, v0n, v1n;
        asm volatile("ds_read_b32 %0, %1" : "=v"(v0) : "v"(v_addr(0, 0)));
        asm volatile("ds_read_b32 %0, %1" : "=v"(v1) : "v"(v_addr(0, 1)));
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(v0), "+v"(v1));
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if (r + 1 < 16) {
                const int rsn = ((r + 1) & 3) + 8 * ((r + 1) >> 2);
                asm volatile("ds_read_b32 %0, %1" : "=v"(v0n) : "v"(v_addr(rsn, 0)));
                asm volatile("ds_read_b32 %0, %1" : "=v"(v1n) : "v"(v_addr(rsn, 1)));
            }
            __builtin_amdgcn_sched_barrier(0);
            o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(v0, s[r], o0, 0, 0, 0);
            if (more && (r & 1) == 0) dma_piece(kbase, Kb, key0 + NWAVE * KT, r >> 1);
            o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(v1, s[r], o1, 0, 0, 0);
            if (r + 1 < 16) {
                __builtin_amdgcn_sched_barrier(0);
                asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(v0n), "+v"(v1n));
                v0 = v0n;
                v1 = v1n;
            }
        }
    }

    // merge the four key-stream states through LDS: flash_attention_kernel's (every wave's DMA is drained: a wave leaves
    // the loop with nothing in flight, and the barrier comes with hipcc's vmcnt(0))
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    float* Os = lds;                               // [NWAVE][QT][O_LD]
    float* Ms = lds + NWAVE * QT * O_LD;           // [NWAVE][QT]
    float* Ls = Ms + NWAVE * QT;                   // [NWAVE][QT]
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int dd = (r & 3) + 8 * (r >> 2) + 4 * half;
        Os[(wave * QT + lq) * O_LD + dd] = o0[r];
        Os[(wave * QT + lq) * O_LD + 32 + dd] = o1[r];
    }
    if (half == 0) {
        Ms[wave * QT + lq] = m_run;
        Ls[wave * QT + lq] = l_run;
    }
    __syncthreads();
    {
        const int dd = tid & 63;
        const int qg = tid >> 6;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int q = qg * 8 + i;
            const int qrow = q0 + q;
            float M = Ms[q];
#pragma unroll
            for (int w = 1; w < NWAVE; ++w) M = fmaxf(M, Ms[w * QT + q]);
            float L = 0.f, acc = 0.f;
#pragma unroll
            for (int w = 0; w < NWAVE; ++w) {
                const float mw = Ms[w * QT + q];
                const float e = mw == -INFINITY ? 0.f : expf(mw - M);     // a stream without keys (short inputs)
                L += e * Ls[w * QT + q];
                acc += e * Os[(w * QT + q) * O_LD + dd];
            }
            if (qrow < a.Tq) aout[(long)qrow * a.ldo + head * 64 + dd] = acc / L;
        }
    }
}

// folds the k_splits partial softmax states of every (query row, head): out = sum_s e^{m_s-M} O_s / sum_s e^{m_s-M} l_s
__global__ __launch_bounds__(64) void flash_merge_kernel(FlashArgs a) {
    WLK_PIN_FLASH_ARGS(a);
    const int row = blockIdx.x, head = blockIdx.y, dd = threadIdx.x;
    const bool batched = a.batch > 0;
    float* const aout = batched ? table_at(a.z.out, blockIdx.z) : a.out;
    const float* const part_o = batched ? table_at(a.z.res, blockIdx.z) : a.part_o;
    const float* const part_m = batched ? part_o + (size_t)a.Tq * a.n_head * a.k_splits * 64 : a.part_m;
    const float* const part_l = batched ? part_m + (size_t)a.Tq * a.n_head * a.k_splits : a.part_l;
    const long base = ((long)row * a.n_head + head) * a.k_splits;
    float M = -INFINITY;
    for (int s = 0; s < a.k_splits; ++s) M = fmaxf(M, part_m[base + s]);
    float L = 0.f, acc = 0.f;
    for (int s = 0; s < a.k_splits; ++s) {
        const float ms = part_m[base + s];
        const float f = ms == -INFINITY ? 0.f : expf(ms - M);
        L += part_l[base + s] * f;
        acc += part_o[(base + s) * 64 + dd] * f;
    }
    aout[(long)row * a.ldo + head * 64 + dd] = acc / L;
}

static void launch_enc_pw(const LaunchCtx& ctx, const FlashArgs& a, const char* tag) {
    const size_t lds = 64 * 1024;            // 4 waves x (8 KiB K + 8 KiB V); the merge (34 KiB) reuses it
    static std::atomic<bool> attr_set[64];
    int dev = 0;
    WLK_HIP(hipGetDevice(&dev));
    if (dev < 64 && !attr_set[dev].load(std::memory_order_acquire)) {
        WLK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(enc_attention_pw_kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        attr_set[dev].store(true, std::memory_order_release);
    }
    const int q_tiles = (a.Tq + QT - 1) / QT;
    const double nb = std::max(a.batch, 1);
    KernelScope ks(ctx, tag, nb * 4.0 * a.Tq * (double)a.Tk * 64.0 * a.n_head,
                   nb * 4.0 * 64.0 * a.n_head * (2.0 * a.Tq + 2.0 * a.Tk));
    hipLaunchKernelGGL(enc_attention_pw_kernel, dim3(q_tiles * a.n_head, std::max(a.batch, 1)), dim3(256), lds, ctx.stream, a);
    WLK_HIP(hipGetLastError());
}

static void launch_flash(const LaunchCtx& ctx, const FlashArgs& a, const char* tag) {
    // sessions launch from different host threads: the per-device "attribute set" marks are atomics (the call itself
    // is idempotent, so a benign double set is all a race can cause)
    static std::atomic<bool> attr_set[64];
    int dev = 0;
    WLK_HIP(hipGetDevice(&dev));
    const size_t lds = kAttnLdsTotal * sizeof(float);
    if (dev < 64 && !attr_set[dev].load(std::memory_order_acquire)) {
        WLK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(flash_attention_kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        attr_set[dev].store(true, std::memory_order_release);
    }
    if (a.head_rank && a.Tk % 4 != 0) throw std::invalid_argument("flash attention: score dump needs Tk % 4 == 0");
    const int q_tiles = (a.Tq + QT - 1) / QT;
    // QK^T and PV: 2 * Tq*Tk*64 MACs per head each; reads q,k,v once, writes out
    const double nb = std::max(a.batch, 1);
    KernelScope ks(ctx, tag, nb * 4.0 * a.Tq * (double)a.Tk * 64.0 * a.n_head,
                   nb * 4.0 * 64.0 * a.n_head * (2.0 * a.Tq + 2.0 * a.Tk));
    if (a.batch > 0 && (a.k_splits > 1 || a.head_rank)) throw std::invalid_argument("flash attention: plain form only when batched");
    // no empty key range: a range is whole 128-key iterations, so 1500 keys are at most 12 ranges (a range without keys
    // would hand the merge a (-inf, 0) state to fold)
    FlashArgs b = a;
    if (b.k_splits > 1) {
        const int n_iter_all = (b.Tk + NWAVE * KT - 1) / (NWAVE * KT);
        const int it_per = (n_iter_all + b.k_splits - 1) / b.k_splits;
        b.k_splits = (n_iter_all + it_per - 1) / it_per;
    }
    hipLaunchKernelGGL(flash_attention_kernel, dim3(q_tiles * b.n_head * b.k_splits, std::max(b.batch, 1)), dim3(256), lds,
                       ctx.stream, b);
    WLK_HIP(hipGetLastError());
    if (b.k_splits > 1) {
        hipLaunchKernelGGL(flash_merge_kernel, dim3(b.Tq, b.n_head), dim3(64), 0, ctx.stream, b);
        WLK_HIP(hipGetLastError());
    }
}

size_t flash_split_scratch_floats(int rows, int n_head, int k_splits) {
    return (size_t)rows * n_head * k_splits * (64 + 2);
}

void launch_encoder_attention(const LaunchCtx& ctx, const float* qkv, float* out, int T, int d, int n_head) {
    FlashArgs a;
    a.q = qkv; a.ldq = 3L * d; a.k = qkv + d; a.v = qkv + 2 * d; a.ldkv = 3L * d; a.out = out; a.ldo = d;
    a.Tq = T; a.Tk = T; a.n_head = n_head;
    launch_enc_pw(ctx, a, "enc_attention");
}

void launch_encoder_attention_batched(const LaunchCtx& ctx, const PtrTable& z, int batch, int T, int d, int n_head) {
    if (batch < 1 || batch > kMaxBatch) throw std::invalid_argument("encoder attention: bad batch");
    FlashArgs a;
    a.ldq = 3L * d; a.ldkv = 3L * d; a.ldo = d; a.Tq = T; a.Tk = T; a.n_head = n_head;
    a.batch = batch; a.z = z; a.z_k_off = d; a.z_v_off = 2L * d;
    launch_enc_pw(ctx, a, "enc_attention");
}

void launch_prefill_cross_attention(const LaunchCtx& ctx, const FlashArgs& a) { launch_flash(ctx, a, "dec_cross_attention_prefill"); }

// in-place softmax of the raw alignment-head scores the prefill dumped: one workgroup per
// (query row, alignment rank) - exactly F.softmax(qk, dim=-1) of simul_whisper.py:411
__global__ __launch_bounds__(256) void ring_softmax_kernel(float* ring, const int* ring_row, const int* beam_of_row,
                                                           const int* ranks, int ring_rows, int n_beam, int T) {
    __shared__ float red[8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = blockIdx.x;
    const int rank = ranks[blockIdx.y];
    float* x = ring + (((long)rank * n_beam + beam_of_row[row]) * ring_rows + ring_row[row]) * (long)T;
    float mx = -INFINITY;
    for (int j = tid; j < T; j += 256) mx = fmaxf(mx, x[j]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float sum = 0.f;
    for (int j = tid; j < T; j += 256) {
        const float e = expf(x[j] - mx);
        x[j] = e;
        sum += e;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off, 64);
    if (lane == 0) red[4 + wave] = sum;
    __syncthreads();
    sum = (red[4] + red[5]) + (red[6] + red[7]);
    for (int j = tid; j < T; j += 256) x[j] = x[j] / sum;
}

void launch_ring_softmax(const LaunchCtx& ctx, float* ring, const int* ring_row, const int* beam_of_row,
                         const int* ranks_dev, int n_ranks, int rows, int ring_rows, int n_beam, int T) {
    if (n_ranks <= 0 || rows <= 0) return;
    KernelScope ks(ctx, "align_ring_softmax", 0.0, 4.0 * 2.0 * rows * (double)n_ranks * T);
    hipLaunchKernelGGL(ring_softmax_kernel, dim3(rows, n_ranks), dim3(256), 0, ctx.stream, ring, ring_row,
                       beam_of_row, ranks_dev, ring_rows, n_beam, T);
    WLK_HIP(hipGetLastError());
}

}  // namespace wlk
