// Encoder self-attention on the bf16 matrix cores at fp32 accuracy (x3.h): softmax(Q K^T) V per 64-wide head with Q, K and
// V as three bf16 planes each, six bf16 MFMAs per fp32 product, fp32 accumulation, fp32 softmax.  gfx950 only.
// Replaces whisper/model.py:148-173 (qkv_attention) for the encoder, as enc_attention_pw_kernel (attention.hip) does
// with fp32 MFMAs: 4.6 GFLOP per launch on base.en took 72 us there (0.40 of the fp32 matrix peak, 31 % of an encode).
//
// Operands come straight from the qkv projection's epilogue (gemm_x3.hip, X3GemmArgs::x3_out):
//   Q | K : X3 rows [T][2 d] (chunks run along the feature axis) - a lane's A / B fragment is one 16-byte unit;
//   V^T   : X3 rows [d][T padded to 32] - chunks run along the KEY axis; stored chunk u of every 32-key group holds keys
//           4 u .. 4 u + 3 and 16 + 4 u .. 16 + 4 u + 3: exactly the keys whose probabilities a lane of group u holds
//           after S^T = K Q^T, so the accumulator registers of step 1 are (after the split into planes) the B operand of
//           step 2 without any data movement between lanes.
// Workgroup = (head, 64 queries), eight waves, all of them computing: wave (qs, ks) owns queries 16 qs .. 16 qs + 15 and
// the key tiles t = ks (mod 2) (flash-style online softmax per wave, the two key streams of a query block merged at the
// end); every wave also issues an eighth - six 1 KiB pieces - of the LDS-DMA that feeds a ring of three slots of two 32-key tiles (K tile
// 12 KiB + V^T tile 12 KiB per stream); one workgroup barrier per pair of tiles.  Per tile and wave: 24
// v_mfma_f32_16x16x32_bf16 for S^T, 24 for O^T += V^T P^T, an 8-value softmax per lane in between.
#include <atomic>
#include <cstdlib>
#include <type_traits>

#include "common.h"
#include "wave_ops.h"
#include "x3.h"

namespace wlk {

namespace {
typedef float af32x4 __attribute__((ext_vector_type(4)));

constexpr int AX_QT = 64, AX_KT = 32;
constexpr int AX_K_ROW = 384;                              // K tile row: 8 chunks x 3 planes x 16 bytes
constexpr int AX_V_ROW = 192;                              // V^T tile row: 4 stored chunks x 3 planes x 16 bytes
constexpr int AX_K_BYTES = AX_KT * AX_K_ROW;               // 12 288
constexpr int AX_V_BYTES = 64 * AX_V_ROW;                  // 12 288
constexpr int AX_TILE_BYTES = AX_K_BYTES + AX_V_BYTES;     // one stream's tile
constexpr int AX_SLOT_BYTES = 2 * AX_TILE_BYTES;           // both streams: 49 152
constexpr int AX_NB = 3, AX_DT = AX_NB - 1;
constexpr int AX_NPW = AX_SLOT_BYTES / 1024 / 8;           // 6 DMA pieces per wave and slot
constexpr size_t AX_LDS_BYTES = (size_t)AX_NB * AX_SLOT_BYTES;
constexpr int AX_PA[6] = {2, 0, 1, 1, 0, 0}, AX_PB[6] = {0, 2, 1, 0, 1, 0};   // plane products, small terms first

template <int N, int I = 0, typename F>
__device__ __forceinline__ void ax_static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        ax_static_for<N, I + 1>(f);
    }
}
// one fragment read: the lane's base register plus a compile-time byte offset in the instruction's 16-bit offset field
template <int OFF>
__device__ __forceinline__ void ax_read(af32x4& f, unsigned base) {
    static_assert(OFF >= 0 && OFF < 65536, "ds_read_b128 offset field");
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(f) : "v"(base), "n"(OFF));
}
__device__ __forceinline__ void ax_wait12(af32x4 (&f)[12]) {
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]), "+v"(f[4]), "+v"(f[5]));
    asm volatile("" : "+v"(f[6]), "+v"(f[7]), "+v"(f[8]), "+v"(f[9]), "+v"(f[10]), "+v"(f[11]));
}
// eight fp32 values -> their three bf16 planes as MFMA operands
__device__ __forceinline__ void ax_split8(const float (&v)[8], bf16x8 (&out)[3]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const X3Triple t = x3_split(v[e]);
        out[0][e] = t.h;
        out[1][e] = t.m;
        out[2][e] = t.l;
    }
}
// key row (relative to the start of its 32-key group) of element e of stored chunk u of V^T: a lane of group u = lane >> 4
// holds, after S^T = K Q^T with 16 x 16 MFMAs, the probabilities of keys 4 u .. 4 u + 3 and 16 + 4 u .. 16 + 4 u + 3
__host__ __device__ inline int ax_vt_key(int u, int e) { return 4 * u + (e & 3) + 16 * (e >> 2); }

// ---- the address sequence of a workgroup, stated once: the kernel and wlk_diag_attn_x3_addresses both call these ------------
// All offsets are bytes from the start of the operand image (qk3).
struct AxGeom {
    int T, n_tiles, n_steps;     // n_steps pairs of 32-key tiles: stream 0 takes tile 2 j, stream 1 tile 2 j + 1
    long row_qk, row_vt;         // bytes of one X3 row of q | k and of V^T
    long q_base;                 // this head's first q chunk in row 0
    long k_base;                 // this head's first k chunk in row 0
    long vt_base;                // V^T row head * 64, stored key chunk 0
};
__host__ __device__ inline int ax_min(int a, int b) { return a < b ? a : b; }
__host__ __device__ inline AxGeom ax_geom(int T, int d, int head, long ldqk, long vt_off, long vt_ld) {
    AxGeom g;
    g.T = T;
    g.n_tiles = (T + AX_KT - 1) / AX_KT;
    g.n_steps = (g.n_tiles + 1) / 2;
    g.row_qk = 3 * ldqk * 2;
    g.row_vt = 3 * vt_ld * 2;
    g.q_base = (long)(head * 8) * 48;
    g.k_base = (long)(d / 8 + head * 8) * 48;
    g.vt_base = 2 * vt_off + (long)(head * 64) * g.row_vt;
    return g;
}
// Q fragment (kstep, plane p) of the lane with query column c and chunk group g of query block qs of the tile at q0
__host__ __device__ inline long ax_q_src(const AxGeom& G, int q0, int qs, int c, int g, int kstep, int p) {
    return G.q_base + (long)ax_min(q0 + 16 * qs + c, G.T - 1) * G.row_qk + ((4 * kstep + g) * 3 + p) * 16;
}
// DMA piece i of wave `wave` covers bytes [1024 j, 1024 j + 1024) of a slot, j = wave + 8 i; lane l moves 16 of them
__host__ __device__ inline int ax_piece_lds(int wave, int lane, int i) { return (wave + 8 * i) * 1024 + 16 * lane; }
// a piece lies inside one of the four 12 KiB regions of a slot: [stream 0: K | V^T][stream 1: K | V^T]
__host__ __device__ inline bool ax_piece_is_k(int wave, int i) { return ((wave + 8 * i) / (AX_K_BYTES / 1024)) % 2 == 0; }
// what that lane fetches for key pair sc (0 <= sc < n_steps); the bank swizzle lives in the source address (K: chunk ^
// (row & 7), V^T: chunk ^ ((row >> 1) & 3), planes in place).  The clamps act on the last pair only: keys past T - 1 read row
// T - 1 (masked in the scores), and a second stream without a tile (odd tile count) re-reads its last real tile.
__host__ __device__ inline long ax_piece_src(const AxGeom& G, int wave, int lane, int i, int sc) {
    const int byte = ax_piece_lds(wave, lane, i);
    const int stream = byte / AX_TILE_BYTES, in_tile = byte - stream * AX_TILE_BYTES;
    if (in_tile < AX_K_BYTES) {
        const int row = in_tile / AX_K_ROW;
        const int up = (in_tile - row * AX_K_ROW) >> 4;
        const int unit = ((up / 3) ^ (row & 7)) * 3 + up % 3;
        const int key = ax_min((2 * sc + stream) * AX_KT + row, G.T - 1);
        return G.k_base + unit * 16 + (long)key * G.row_qk;
    }
    const int off = in_tile - AX_K_BYTES;
    const int row = off / AX_V_ROW;
    const int up = (off - row * AX_V_ROW) >> 4;
    const int unit = ((up / 3) ^ ((row >> 1) & 3)) * 3 + up % 3;
    const int pair = ax_min(sc, (G.n_tiles - 1 - stream) / 2);
    return G.vt_base + (long)row * G.row_vt + unit * 16 + (long)(2 * pair + stream) * (AX_KT / 8) * 48;
}
// Before the last pair no clamp acts, and a piece's source moves by a wave-uniform stride per step: two tiles of K rows, or
// eight stored chunks of a V^T row
__host__ __device__ inline long ax_piece_stride(const AxGeom& G, int wave, int i) {
    return ax_piece_is_k(wave, i) ? 2L * AX_KT * G.row_qk : 2L * (AX_KT / 8) * 48;
}
// The request of ring step `step` (0 .. n_steps + 1; the two past the end re-fetch the last pair into a free slot), as the
// kernel forms it: a pointer that advances while step < n_steps - 1, the last pair's own pointer from then on
__host__ __device__ inline long ax_piece_src_at_step(const AxGeom& G, int wave, int lane, int i, int step) {
    return step < G.n_steps - 1 ? ax_piece_src(G, wave, lane, i, 0) + step * ax_piece_stride(G, wave, i)
                                : ax_piece_src(G, wave, lane, i, G.n_steps - 1);
}
// Fragment reads, relative to the slot: lane (c = lane & 15, g = lane >> 4) of key stream ks reads K fragment (kb, kstep, p) at
// ax_k_frag(ks, c, g, kstep) + kb * AX_K_KB + p * 16 and V^T fragment (db, p) at ax_v_frag(ks, c, g) + db * AX_V_DB + p * 16:
// neither swizzle term, row & 7 nor (row >> 1) & 3, changes with kb or db (rows 16 kb + c, 16 db + c)
constexpr int AX_K_KB = 16 * AX_K_ROW, AX_V_DB = 16 * AX_V_ROW;
__host__ __device__ inline unsigned ax_k_frag(int ks, int c, int g, int kstep) {
    return (unsigned)(ks * AX_TILE_BYTES + c * AX_K_ROW + (((4 * kstep + g) ^ (c & 7)) * 3) * 16);
}
__host__ __device__ inline unsigned ax_v_frag(int ks, int c, int g) {
    return (unsigned)(ks * AX_TILE_BYTES + AX_K_BYTES + c * AX_V_ROW + ((g ^ ((c >> 1) & 3)) * 3) * 16);
}
}  // namespace

struct AttnX3Args {
    const unsigned short* qk3;   // X3 rows [T][ldqk]: columns [0, d) = q (pre-scaled), [d, 2 d) = k (pre-scaled)
    long ldqk;                   // fp32-element units (2 d)
    long vt_off;                 // V^T = qk3 + vt_off (bf16 units): X3 rows [d][vt_ld], chunks along the keys
    long vt_ld;
    float* out;                  // [T][ldo] fp32
    long ldo;
    int T, d, n_head;
    int batch;
    int x3_out;                  // round 6: != 0 -> `out` (z.out[i]) is an X3 row image [T][ldo] (three bf16 planes, x3.h) instead of
                                 // fp32 rows: the operand of an X3 out projection (d >= 1024 models), no fp32 copy, no pack launch
    PtrTable z;                  // batched encodes: qk3 = z.in[i], out = z.out[i]
};

// Round 4, second version.  The first one had four compute waves (32 queries each, 32 x 32 MFMAs) beside four loader
// waves: per key tile a compute wave ran its S MFMAs, ~220 VALU instructions of softmax / plane split and its P V MFMAs
// strictly one after the other, so the matrix pipe of its SIMD idled through every softmax (47 us per launch against
// 18 us of MFMA time).  Here ALL EIGHT waves compute: wave (qs, ks) owns 16 queries (v_mfma_f32_16x16x32_bf16: same flop
// rate, half the accumulator and softmax work per wave) of key stream ks, the two waves of a SIMD belong to different
// streams and cover each other's softmax and DMA issue (6 pieces per wave and step) with their MFMAs.
__global__ __launch_bounds__(512) void enc_attention_x3_kernel(AttnX3Args a) {
    asm volatile("" ::"s"(a.qk3), "s"(a.ldqk), "s"(a.vt_off), "s"(a.vt_ld), "s"(a.out), "s"(a.ldo), "s"(a.T), "s"(a.d), "s"(a.n_head),
                 "s"(a.batch));
    __builtin_amdgcn_sched_barrier(0);
    extern __shared__ __attribute__((aligned(1024))) unsigned char lds[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool batched = a.batch > 0;
    const unsigned short* const qk3 = batched ? reinterpret_cast<const unsigned short*>(table_at(a.z.in, blockIdx.y)) : a.qk3;
    float* const aout = batched ? table_at(a.z.out, blockIdx.y) : a.out;
    const int T = a.T;
    const int head = blockIdx.x % a.n_head;          // head == XCD for 8 heads: a head's K / V stay in one L2
    const int q0 = (blockIdx.x / a.n_head) * AX_QT;
    const AxGeom G = ax_geom(T, a.d, head, a.ldqk, a.vt_off, a.vt_ld);
    const int n_tiles = G.n_tiles, n_steps = G.n_steps;
    const int qs = wave & 3, ks = wave >> 2;
    const int c = lane & 15, g = lane >> 4;
    const char* const image = reinterpret_cast<const char*>(qk3);

    // Q fragments (B operand of S^T = K Q^T): query q0 + 16 qs + c, feature chunk 4 kstep + g, plane p - first in the queue
    bf16x8 qf[6];
#pragma unroll
    for (int kstep = 0; kstep < 2; ++kstep)
#pragma unroll
        for (int p = 0; p < 3; ++p)
            qf[kstep * 3 + p] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const x3_u32x4*>(image + ax_q_src(G, q0, qs, c, g, kstep, p)));
    // ---- DMA sources (ax_piece_src_at_step): each of the wave's six pieces keeps a per-lane pointer that a wave-uniform
    // stride advances once per step, and the pointer of the last pair - the only one the clamps act on -, which also serves
    // the two tail fetches.  Nothing is multiplied in the key loop. ---------------------------------------------------------
    const char* cur[AX_NPW];
    const char* last[AX_NPW];
    long stride[AX_NPW];
#pragma unroll
    for (int i = 0; i < AX_NPW; ++i) {
        cur[i] = image + ax_piece_src(G, wave, lane, i, 0);
        last[i] = image + ax_piece_src(G, wave, lane, i, n_steps - 1);
        stride[i] = ax_piece_stride(G, wave, i);
    }
    unsigned dma_slot = 0;                              // byte offset of the slot the next issue fills: a counter, not step % 3
    auto issue_step = [&](int step) {
        const unsigned dst = dma_slot;
        dma_slot = dma_slot == (AX_NB - 1) * AX_SLOT_BYTES ? 0u : dma_slot + AX_SLOT_BYTES;
        if (step < n_steps - 1) {                       // wave-uniform
            ax_static_for<AX_NPW>([&](auto I) {
                constexpr int i = decltype(I)::value;
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)cur[i],
                                                 (__attribute__((address_space(3))) void*)(lds + dst + (wave + 8 * i) * 1024), 16, 0, 0);
                cur[i] += stride[i];
            });
        } else {
            ax_static_for<AX_NPW>([&](auto I) {
                constexpr int i = decltype(I)::value;
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)last[i],
                                                 (__attribute__((address_space(3))) void*)(lds + dst + (wave + 8 * i) * 1024), 16, 0, 0);
            });
        }
    };
    issue_step(0);
    issue_step(1);

    // ---- fragment addresses of this wave's stream: two base registers for K (kstep 0 / 1) and one for V^T; kb, db and the
    // plane are immediates of the reads --------------------------------------------------------------------------------
    const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)lds;
    const unsigned k_base0 = lds_base + ax_k_frag(ks, c, g, 0), k_base1 = lds_base + ax_k_frag(ks, c, g, 1);
    const unsigned v_base = lds_base + ax_v_frag(ks, c, g);
    af32x4 o[4];
#pragma unroll
    for (int db = 0; db < 4; ++db) o[db] = af32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;

    // (Measured and dropped, profiles/r04j_x3_attention_ablation.txt, r04k_x3_attention_skewed_ablation.txt: running stream 1 half a step out of phase - it finishes
    // tile st - 1 while stream 0 computes S(st) - so that one wave of a SIMD is in its softmax while the other is in its
    // MFMAs: 60.8 us instead of 48.9.  What the two waves of a SIMD share is issue bandwidth, not just the matrix pipe.)
    af32x4 vf[12];
    float s[8];
    auto phase_s = [&](int tile, unsigned off, int next) {   // fragments of `tile` (slot at byte `off`) -> registers, pair `next` requested, s = K Q^T
        af32x4 kf[12];
        const unsigned k0 = k_base0 + off, k1 = k_base1 + off, vb = v_base + off;
        ax_static_for<12>([&](auto X) {
            constexpr int t = decltype(X)::value;
            constexpr int kb = t / 6, kstep = (t / 3) % 2, p = t % 3;
            ax_read<kb * AX_K_KB + p * 16>(kf[t], kstep ? k1 : k0);
        });
        ax_static_for<12>([&](auto X) {
            constexpr int t = decltype(X)::value;
            constexpr int db = t / 3, p = t % 3;
            ax_read<db * AX_V_DB + p * 16>(vf[t], vb);
        });
        // The DMA of pair `next` goes out here, behind the reads and in front of the wait for them: its issue cost hides in the
        // LDS latency (measured against the top of the step, between S and P V, and the end of the step: DESIGN section 12)
        issue_step(next);
        ax_wait12(kf);
        // key blocks 0 / 1 are two independent accumulator chains
        af32x4 s2[2] = {af32x4{0.f, 0.f, 0.f, 0.f}, af32x4{0.f, 0.f, 0.f, 0.f}};
        ax_static_for<24>([&](auto X) {
            constexpr int x = decltype(X)::value;
            constexpr int t = x / 4, kstep = (x / 2) % 2, kb = x % 2;      // product t of feature step kstep, key block kb
            s2[kb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, kf[kb * 6 + kstep * 3 + AX_PA[t]]),
                                                             qf[kstep * 3 + AX_PB[t]], s2[kb], 0, 0, 0);
        });
        // s[4 kb + i] = score of key key0 + 16 kb + 4 g + i against this lane's query
#pragma unroll
        for (int i = 0; i < 4; ++i) { s[i] = s2[0][i]; s[4 + i] = s2[1][i]; }
        const int key0 = tile * AX_KT;
        if (__builtin_amdgcn_readfirstlane(key0 + AX_KT > T)) {      // only the last tile has keys past the end
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (key0 + 16 * (i >> 2) + 4 * g + (i & 3) >= T) s[i] = -INFINITY;
        }
        ax_wait12(vf);
    };
    auto phase_pv = [&]() {                                 // online softmax of s, O^T += V^T P^T
        bf16x8 pf[3];
        // this lane's query column: its 8 keys here, the others in lanes ^ 16, ^ 32
        float mt = fmaxf(fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3])), fmaxf(fmaxf(s[4], s[5]), fmaxf(s[6], s[7])));
        mt = fmaxf(mt, wave_xor<16>(mt));
        mt = fmaxf(mt, wave_xor<32>(mt));
        const float m_new = fmaxf(m_run, mt);
        const float alpha = __expf(m_run - m_new);
        float rs = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            s[i] = __expf(s[i] - m_new);
            rs += s[i];
        }
        rs += wave_xor<16>(rs);
        rs += wave_xor<32>(rs);
        l_run = l_run * alpha + rs;
        m_run = m_new;
        if (__builtin_amdgcn_ballot_w64(alpha != 1.0f) != 0) {
#pragma unroll
            for (int db = 0; db < 4; ++db) o[db] *= alpha;
        }
        // the lane's 8 probabilities are, split into planes, its B fragment
        ax_split8(s, pf);
        ax_static_for<24>([&](auto X) {
            constexpr int x = decltype(X)::value;
            constexpr int t = x / 4, db = x % 4;      // product t of feature block db: four independent chains
            o[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, vf[db * 3 + AX_PA[t]]), pf[AX_PB[t]], o[db], 0, 0, 0);
        });
    };

    asm volatile("s_waitcnt vmcnt(6)" ::: "memory");      // the Q fragments and this wave's pieces of pair 0
    // the Q fragments are in their registers from here on: said to the compiler outside the loop, or it waits for them - and
    // with them for every DMA piece in flight - in front of the first MFMA of every step
    asm volatile("" : "+v"(qf[0]), "+v"(qf[1]), "+v"(qf[2]), "+v"(qf[3]), "+v"(qf[4]), "+v"(qf[5]));
    __builtin_amdgcn_s_barrier();
    unsigned off = 0;                          // byte offset of the slot of pair st
    for (int st = 0; st < n_steps; ++st) {
        const int tile = 2 * st + ks;
        if (tile < n_tiles) {      // wave-uniform
            phase_s(tile, off, st + AX_DT);
            phase_pv();
        } else {
            issue_step(st + AX_DT);      // a second stream without a tile still feeds the ring
        }
        off = off == (AX_NB - 1) * AX_SLOT_BYTES ? 0u : off + AX_SLOT_BYTES;
        asm volatile("s_waitcnt vmcnt(6) lgkmcnt(0)" ::: "memory");   // this wave's pieces of pair st + 1 have landed
        __builtin_amdgcn_s_barrier();          // pair st + 1 readable; everybody is done with pair st's LDS image
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();              // the tail fetches have landed: the ring can be reused

    // ---- merge the two key streams of each 16-query block through LDS and write the normalised rows -------------------
    // o[db][i] is O^T[feature 16 db + 4 g + i][query c]
    constexpr int O_LD = 68;
    float* Os = reinterpret_cast<float*>(lds);                 // [wave][16 queries][O_LD]
    float* Ms = Os + 8 * 16 * O_LD;                            // [wave][16]
    float* Ls = Ms + 8 * 16;
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
        for (int i = 0; i < 4; ++i) Os[(wave * 16 + c) * O_LD + 16 * db + 4 * g + i] = o[db][i];
    if (g == 0) {
        Ms[wave * 16 + c] = m_run;
        Ls[wave * 16 + c] = l_run;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (a.x3_out) {
        // one (query, 8-feature chunk) per thread: 64 queries x 8 chunks = the 512 threads; same merge arithmetic per element
        const int tid = threadIdx.x;
        const int q = tid >> 3, ch = tid & 7;
        const int qrow = q0 + q;
        const int w0 = q >> 4, w1 = w0 + 4;
        const float m0 = Ms[w0 * 16 + (q & 15)], m1 = Ms[w1 * 16 + (q & 15)];
        const float M = fmaxf(m0, m1);
        const float e0 = m0 == -INFINITY ? 0.f : expf(m0 - M), e1 = m1 == -INFINITY ? 0.f : expf(m1 - M);
        const float L = e0 * Ls[w0 * 16 + (q & 15)] + e1 * Ls[w1 * 16 + (q & 15)];
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int dd = 8 * ch + e;
            v[e] = (e0 * Os[(w0 * 16 + (q & 15)) * O_LD + dd] + e1 * Os[(w1 * 16 + (q & 15)) * O_LD + dd]) / L;
        }
        if (qrow < T)
            x3_store_chunk(reinterpret_cast<unsigned short*>(aout) + (long)qrow * 3 * a.ldo + (long)(head * 8 + ch) * 24, v);
    } else {
        const int tid = threadIdx.x;       // 0 .. 511
        const int dd = tid & 63, qg = tid >> 6;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int q = qg * 8 + i;      // 0 .. 63: 16-query block q >> 4, row q & 15
            const int qrow = q0 + q;
            const int w0 = q >> 4, w1 = w0 + 4;      // the block's two streams (wave = qs + 4 ks)
            const float m0 = Ms[w0 * 16 + (q & 15)], m1 = Ms[w1 * 16 + (q & 15)];
            const float M = fmaxf(m0, m1);
            const float e0 = m0 == -INFINITY ? 0.f : expf(m0 - M), e1 = m1 == -INFINITY ? 0.f : expf(m1 - M);
            const float L = e0 * Ls[w0 * 16 + (q & 15)] + e1 * Ls[w1 * 16 + (q & 15)];
            const float acc = e0 * Os[(w0 * 16 + (q & 15)) * O_LD + dd] + e1 * Os[(w1 * 16 + (q & 15)) * O_LD + dd];
            if (qrow < T) aout[(long)qrow * a.ldo + head * 64 + dd] = acc / L;
        }
    }
}

// fp32 qkv [T][3 d] -> the operand image enc_attention_x3_kernel reads (the layout the qkv projection's X3 epilogue
// writes): X3 rows [T][2 d] (q | k), then V^T as X3 rows [d][vt_ld] whose stored chunk u of every 32-key group holds the
// keys 4 u .. 4 u + 3 and 16 + 4 u .. 16 + 4 u + 3 (ax_vt_key).
// Diagnostics only (wlk_diag_encoder_attention_x3): in the product the GEMM epilogue produces this image directly.
__global__ __launch_bounds__(256) void x3_pack_qkv_kernel(const float* __restrict__ qkv, unsigned short* __restrict__ out, int T, int d,
                                                          long vt_off, long vt_ld) {
    const long n_qk = (long)T * (2 * d / 8), n_vt = (long)d * (vt_ld / 8);
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    float v[8];
    if (idx < n_qk) {
        const int row = (int)(idx / (2 * d / 8)), c = (int)(idx - (long)row * (2 * d / 8));
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = qkv[(long)row * 3 * d + 8 * c + e];
        x3_store_chunk(out + (long)row * 3 * (2 * d) + (long)c * 24, v);
    } else if (idx < n_qk + n_vt) {
        const long j = idx - n_qk;
        const int dcol = (int)(j / (vt_ld / 8)), u = (int)(j - (long)dcol * (vt_ld / 8));
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int t = 32 * (u >> 2) + ax_vt_key(u & 3, e);
            v[e] = t < T ? qkv[(long)t * 3 * d + 2 * d + dcol] : 0.f;
        }
        x3_store_chunk(out + vt_off + (long)dcol * 3 * vt_ld + (long)u * 24, v);
    }
}

void launch_x3_pack_qkv(const LaunchCtx& ctx, const float* qkv, unsigned short* out, int T, int d, long vt_off, long vt_ld) {
    const long n = (long)T * (2 * d / 8) + (long)d * (vt_ld / 8);
    KernelScope ks(ctx, "x3_pack_qkv");
    hipLaunchKernelGGL(x3_pack_qkv_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx.stream, qkv, out, T, d, vt_off, vt_ld);
    WLK_HIP(hipGetLastError());
}

bool enc_attention_x3_enabled() {
    static const bool on = [] {
        const char* e = getenv("WLK_X3_ATTN");
        return !(e && e[0] == '0');
    }();
    return on;
}

// what launch_encoder_attention_x3 refuses (the launcher calls it first; wlk_diag_enc_op before it uploads anything)
void enc_attention_x3_check(long ldqk, long vt_ld, long ldo, int T, int d, int n_head, bool x3_out) {
    if (d != n_head * 64 || ldqk % 8 != 0 || vt_ld % 32 != 0 || vt_ld < ((T + 31) / 32) * 32 || T < 64)
        throw std::invalid_argument("x3 attention: unsupported shape");
    if (x3_out && ldo % 8 != 0) throw std::invalid_argument("x3 attention: X3 result rows need ldo % 8 == 0");
}

long enc_attention_x3_addresses(int T, int d, int n_head, int head, int q_tile, long* src, int* dst, long cap) {
    enc_attention_x3_check(2L * d, x3_attn_vt_ld(T), d, T, d, n_head, false);
    if (head < 0 || head >= n_head || q_tile < 0 || q_tile >= (T + AX_QT - 1) / AX_QT)
        throw std::invalid_argument("x3 attention addresses: no such workgroup");
    const AxGeom G = ax_geom(T, d, head, 2L * d, x3_attn_vt_off(T, d), x3_attn_vt_ld(T));
    long n = 0;
    auto put = [&](long s, int l) {
        if (n < cap) { src[n] = s; dst[n] = l; }
        ++n;
    };
    for (int tid = 0; tid < 512; ++tid) {
        const int lane = tid & 63, wave = tid >> 6;
        for (int kstep = 0; kstep < 2; ++kstep)
            for (int p = 0; p < 3; ++p) put(ax_q_src(G, q_tile * AX_QT, wave & 3, lane & 15, lane >> 4, kstep, p), -1);
    }
    int slot = 0;                                       // the kernel's counter: issue_step fills slot 0, 1, 2, 0, ...
    for (int step = 0; step < G.n_steps + AX_DT; ++step) {
        for (int wave = 0; wave < 8; ++wave)
            for (int i = 0; i < AX_NPW; ++i)
                for (int lane = 0; lane < 64; ++lane)
                    put(ax_piece_src_at_step(G, wave, lane, i, step), slot * AX_SLOT_BYTES + ax_piece_lds(wave, lane, i));
        slot = slot == AX_NB - 1 ? 0 : slot + 1;
    }
    return n;
}

void launch_encoder_attention_x3(const LaunchCtx& ctx, const unsigned short* qk3, long ldqk, long vt_off, long vt_ld, float* out,
                                 long ldo, int T, int d, int n_head, const PtrTable* z, int batch, bool x3_out) {
    enc_attention_x3_check(ldqk, vt_ld, ldo, T, d, n_head, x3_out);
    static std::atomic<uint64_t> configured{0};
    int dev = 0;
    WLK_HIP(hipGetDevice(&dev));
    if (!(configured.load(std::memory_order_acquire) >> (dev & 63) & 1)) {
        WLK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&enc_attention_x3_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)AX_LDS_BYTES));
        configured.fetch_or(1ull << (dev & 63), std::memory_order_release);
    }
    AttnX3Args a{};
    a.qk3 = qk3; a.ldqk = ldqk; a.vt_off = vt_off; a.vt_ld = vt_ld; a.out = out; a.ldo = ldo; a.T = T; a.d = d; a.n_head = n_head;
    a.batch = batch;
    a.x3_out = x3_out ? 1 : 0;
    if (batch > 0) a.z = *z;
    const int q_tiles = (T + AX_QT - 1) / AX_QT;
    KernelScope ks(ctx, "enc_attention_x3", (batch > 0 ? batch : 1) * 4.0 * (double)T * T * 64 * n_head, 0.0);
    const dim3 grid(q_tiles * n_head, batch > 0 ? batch : 1);
    hipLaunchKernelGGL(enc_attention_x3_kernel, grid, dim3(512), AX_LDS_BYTES, ctx.stream, a);
    WLK_HIP(hipGetLastError());
}

}  // namespace wlk
