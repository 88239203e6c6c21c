// Dynamic time warping over a [tokens, frames] cost matrix: the alignment step of the reference's word timestamps
// (whisper/timing.py:82-105 `dtw_cpu`; the reference's CUDA build runs the same recurrence as a Triton kernel,
// timing.py:108-138).  SURVEY 8(f) rank 4: the one kernel LocalAgreement's batch Whisper needs beyond the encoder /
// decoder kernels of the streaming path.
//
//   cost[i][j] = x[i-1][j-1] + min(cost[i-1][j-1], cost[i-1][j], cost[i][j-1]),   cost[0][0] = 0, borders = inf
//   trace[i][j] = 0 (diagonal) if c0 < c1 and c0 < c2, else 1 (up) if c1 < c0 and c1 < c2, else 2 (left)
//
// exactly dtw_cpu's strict comparisons (ties go left), one fp32 add per cell.  The recurrence is a wavefront: all cells
// of an anti-diagonal i + j = k are independent.  One workgroup, one thread per token row (N <= 1024, the text context
// is 448), N + M - 1 steps with a workgroup barrier each; the three live anti-diagonals sit in LDS, a row's x values
// are read one step ahead, the trace goes out frame-major so that a step's writes are contiguous.  Latency-bound by
// construction (~2000 dependent steps for a 30 s window): what matters is that nothing but the barrier is on the
// step's critical path.
#include <cstdint>
#include <algorithm>
#include <cstring>
#include <mutex>
#include <stdexcept>
#include <vector>

#include "../../include/wlk_hip.h"
#include "common.h"
#include "internal.h"

namespace wlk {

constexpr int kDtwMaxRows = 1024;

// the recurrence of one cost matrix by one workgroup (thread = token row); diag = the three live anti-diagonals in LDS
__device__ __forceinline__ void dtw_wavefront_body(const float* __restrict__ x, int N, int M,
                                                   signed char* __restrict__ trace_t /* [M+1][N+1] */,
                                                   float (*diag)[kDtwMaxRows + 1]) {
    const int i = threadIdx.x + 1;               // token row 1..N of the padded recurrence
    for (int r = threadIdx.x; r < 3 * (kDtwMaxRows + 1); r += blockDim.x) (&diag[0][0])[r] = INFINITY;
    __syncthreads();
    if (threadIdx.x == 0) diag[0][0] = 0.f;      // cost[0][0]; diag[1] = anti-diagonal 1: cost[0][1] = cost[1][0] = inf
    __syncthreads();
    int b2 = 0, b1 = 1, b0 = 2;                  // buffers of k-2, k-1, k
    const bool mine = i <= N;
    const float* xr = x + (long)(mine ? i - 1 : 0) * M;
    float x_next = mine && M > 0 ? xr[0] : 0.f;  // x[i-1][j-1] of this row's next cell
    for (int k = 2; k <= N + M; ++k) {
        const int j = k - i;
        if (mine && j >= 1 && j <= M) {
            const float xv = x_next;
            if (j < M) x_next = xr[j];
            const float c0 = diag[b2][i - 1], c1 = diag[b1][i - 1], c2 = diag[b1][i];
            float c;
            signed char t;
            if (c0 < c1 && c0 < c2) { c = c0; t = 0; }
            else if (c1 < c0 && c1 < c2) { c = c1; t = 1; }
            else { c = c2; t = 2; }
            diag[b0][i] = xv + c;
            trace_t[(long)j * (N + 1) + i] = t;
        }
        if (threadIdx.x == 0) diag[b0][0] = INFINITY;   // cost[0][k]
        __syncthreads();
        const int t = b2; b2 = b1; b1 = b0; b0 = t;
    }
}

__global__ __launch_bounds__(kDtwMaxRows) void dtw_wavefront_kernel(const float* __restrict__ x, int N, int M,
                                                                    signed char* __restrict__ trace_t /* [M+1][N+1] */) {
    __shared__ float diag[3][kDtwMaxRows + 1];   // cost of row i on the anti-diagonals k-2, k-1, k
    dtw_wavefront_body(x, N, M, trace_t, diag);
}

// frame-major [M+1][N+1] -> token-major [N+1][M+1] (the layout dtw_cpu hands to backtrace), 32x32 tiles through LDS
__device__ __forceinline__ void dtw_transpose_body(const signed char* __restrict__ in, signed char* __restrict__ out,
                                                   int rows_in /* M+1 */, int cols_in /* N+1 */, signed char (*tile)[33]) {
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    for (int r = ty; r < 32; r += 8)
        if (r0 + r < rows_in && c0 + tx < cols_in) tile[r][tx] = in[(long)(r0 + r) * cols_in + c0 + tx];
    __syncthreads();
    for (int r = ty; r < 32; r += 8)
        if (c0 + r < cols_in && r0 + tx < rows_in) out[(long)(c0 + r) * rows_in + r0 + tx] = tile[tx][r];
}

__global__ __launch_bounds__(256) void dtw_transpose_kernel(const signed char* __restrict__ in, signed char* __restrict__ out,
                                                            int rows_in /* M+1 */, int cols_in /* N+1 */) {
    __shared__ signed char tile[32][33];
    dtw_transpose_body(in, out, rows_in, cols_in, tile);
}

// ---- up to 8 cost matrices of different shapes at once (wlk_group_find_alignment) ----------------------------------------
// The recurrence is latency-bound on one CU, so the windows run side by side: workgroup = window, shape and pointers
// from the table, the block sized for the tallest window (threads beyond a window's rows only keep its barriers).
__global__ __launch_bounds__(kDtwMaxRows) void dtw_wavefront_ragged_kernel(const AlignWin* __restrict__ tab) {
    __shared__ float diag[3][kDtwMaxRows + 1];
    const AlignWin t = tab[blockIdx.x];
    dtw_wavefront_body(t.cost, t.N, t.F, t.trace_t, diag);
}
__global__ __launch_bounds__(256) void dtw_transpose_ragged_kernel(const AlignWin* __restrict__ tab) {
    __shared__ signed char tile[32][33];
    const AlignWin t = tab[blockIdx.z];
    if ((int)blockIdx.x * 32 > t.N || (int)blockIdx.y * 32 > t.F) return;      // tile outside this window's [F+1][N+1]
    dtw_transpose_body(t.trace_t, t.trace, t.F + 1, t.N + 1, tile);
}

// The path walk of timing.backtrace, reduced to what word_timings reads: starts[i - 1] = frame index (column - 1) of the
// cell at which the path, walked back from (N, M), LEAVES token row i = 1 .. N - the first path element of that text
// index in forward order.  With backtrace's overrides (column 0 only moves up; row 0 only moves left and is not needed
// for the starts) a row's exit is "the largest j' <= j whose code is not LEFT", and the next row is entered at j' - 1
// (diagonal) or j' (up).  No thread follows the path cell by cell through memory: the waves of the workgroup turn the
// codes of a band of rows into two bit masks per 64-cell chunk (one byte load per lane, two ballots: not-left, diagonal)
// in LDS - 2 x 24 KB, 128 rows of a 1500-frame window per band - and one thread then resolves each row of the band with
// a masked count-leading-zeros on LDS words: N + ceil(M / 64) dependent LDS look-ups at most, no dependent global load.
constexpr int kWalkWords = 3072;                 // 64-cell words per mask in LDS
__global__ __launch_bounds__(1024) void dtw_walk_kernel(const AlignWin* __restrict__ tab) {
    __shared__ unsigned long long not_left[kWalkWords], diagonal[kWalkWords];
    const AlignWin t = tab[blockIdx.x];
    const int N = t.N, M = t.F;
    const int W = (M + 64) / 64;                 // words of a row's columns 0 .. M
    const int band = kWalkWords / W;             // rows per band (>= 48: M <= kDtwWalkMaxCols)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    int j = M;                                   // thread 0: the column at which the path enters the next row
    for (int hi = N; hi >= 1; hi -= band) {
        const int lo = hi - band + 1 > 1 ? hi - band + 1 : 1;
        const int chunks = (hi - lo + 1) * W;
        for (int c = wave; c < chunks; c += n_waves) {
            const int i = lo + c / W, col = (c % W) * 64 + lane;
            signed char code = 2;                // beyond column M: left, never an exit
            if (col == 0) code = 1;              // column 0 only moves up
            else if (col <= M) code = t.trace[(long)i * (M + 1) + col];
            const unsigned long long nl = __ballot(code != 2), dg = __ballot(code == 0);
            if (lane == 0) {
                not_left[c] = nl;
                diagonal[c] = dg;
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int i = hi; i >= lo; --i) {
                const unsigned long long* row = not_left + (i - lo) * W;
                int w = j >> 6;
                unsigned long long bits = row[w] & (~0ull >> (63 - (j & 63)));
                while (bits == 0) bits = row[--w];           // ends at the latest in word 0: column 0 is always set
                const int jp = w * 64 + 63 - __clzll((long long)bits);
                t.starts[i - 1] = jp - 1;
                j = jp - (int)((diagonal[(i - lo) * W + w] >> (jp & 63)) & 1ull);
            }
        }
        __syncthreads();
    }
}

// Per-device workspace of wlk_dtw: device buffers and pinned staging that only ever grow, and a non-blocking stream of
// their own - a word-timestamp alignment neither allocates (hipFree synchronises the whole device, i.e. every
// streaming session's encode and decode streams) nor touches the NULL stream.  One alignment at a time per device.
struct DtwWorkspace {
    std::mutex mu;
    hipStream_t stream = nullptr;
    float* xd = nullptr;
    signed char *td = nullptr, *tt = nullptr;
    char* pinned = nullptr;
    size_t x_cap = 0, t_cap = 0, pin_cap = 0;
    void reserve(size_t nx, size_t nt) {
        if (!stream) WLK_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        if (nx > x_cap) {
            if (xd) WLK_HIP(hipFree(xd));
            xd = nullptr; x_cap = 0;
            WLK_HIP(hipMalloc(reinterpret_cast<void**>(&xd), nx * sizeof(float)));
            x_cap = nx;
        }
        if (nt > t_cap) {
            if (td) WLK_HIP(hipFree(td));
            if (tt) WLK_HIP(hipFree(tt));
            td = tt = nullptr; t_cap = 0;
            WLK_HIP(hipMalloc(reinterpret_cast<void**>(&td), nt));
            WLK_HIP(hipMalloc(reinterpret_cast<void**>(&tt), nt));
            t_cap = nt;
        }
        const size_t pin = std::max(nx * sizeof(float), nt);
        if (pin > pin_cap) {
            if (pinned) WLK_HIP(hipHostFree(pinned));
            pinned = nullptr; pin_cap = 0;
            WLK_HIP(hipHostMalloc(reinterpret_cast<void**>(&pinned), pin, hipHostMallocDefault));
            pin_cap = pin;
        }
    }
};
constexpr int kDtwMaxDevices = 64;
static DtwWorkspace g_dtw_ws[kDtwMaxDevices];

// the recurrence + transposition on `stream`: x_dev [N][M] -> trace_dev token-major [(N+1)][(M+1)]; scratch_t [(M+1)(N+1)]
void launch_dtw(hipStream_t stream, const float* x_dev, int n_rows, int n_cols, signed char* scratch_t, signed char* trace_dev) {
    const size_t nt = (size_t)(n_rows + 1) * (n_cols + 1);
    WLK_HIP(hipMemsetAsync(scratch_t, 0xff, nt, stream));   // -1 like dtw_cpu's untouched border cells
    const int threads = std::max(64, ((n_rows + 63) / 64) * 64);
    hipLaunchKernelGGL(dtw_wavefront_kernel, dim3(1), dim3(threads), 0, stream, x_dev, n_rows, n_cols, scratch_t);
    hipLaunchKernelGGL(dtw_transpose_kernel, dim3((n_rows + 1 + 31) / 32, (n_cols + 1 + 31) / 32), dim3(256), 0, stream,
                       scratch_t, trace_dev, n_cols + 1, n_rows + 1);
    WLK_HIP(hipGetLastError());
}

void launch_dtw_ragged(const LaunchCtx& ctx, const AlignWin* tab_dev, const AlignWin* tab_host, int n) {
    if (!tab_dev || !tab_host || n < 1 || n > kAlignWinMax) throw std::invalid_argument("ragged dtw: 1..8 windows");
    int max_n = 0, max_f = 0;
    for (int i = 0; i < n; ++i) {
        const AlignWin& t = tab_host[i];
        if (!t.cost || !t.trace_t || !t.trace || !t.starts) throw std::invalid_argument("ragged dtw: null operand");
        if (t.N < 1 || t.N > kDtwMaxRows || t.F < 1 || t.F > kDtwWalkMaxCols)
            throw std::invalid_argument("ragged dtw: 1..1024 rows and 1..4095 columns");
        max_n = std::max(max_n, t.N); max_f = std::max(max_f, t.F);
    }
    const int threads = std::max(64, ((max_n + 63) / 64) * 64);
    hipLaunchKernelGGL(dtw_wavefront_ragged_kernel, dim3(n), dim3(threads), 0, ctx.stream, tab_dev);
    hipLaunchKernelGGL(dtw_transpose_ragged_kernel, dim3((max_n + 1 + 31) / 32, (max_f + 1 + 31) / 32, n), dim3(256), 0, ctx.stream,
                       tab_dev);
    hipLaunchKernelGGL(dtw_walk_kernel, dim3(n), dim3(1024), 0, ctx.stream, tab_dev);
    WLK_HIP(hipGetLastError());
}

}  // namespace wlk

using namespace wlk;

extern "C" int wlk_dtw(int device, const float* x, int32_t n_rows, int32_t n_cols, int8_t* trace) {
    if (!x || !trace) return fail(WLK_ERR_ARG, "dtw: NULL argument");
    if (n_rows < 1 || n_cols < 1) return fail(WLK_ERR_ARG, "dtw: empty cost matrix");
    if (n_rows > kDtwMaxRows) return fail(WLK_ERR_CAPACITY, "dtw: more than 1024 rows");
    if ((long)n_rows * n_cols > (1L << 28)) return fail(WLK_ERR_CAPACITY, "dtw: cost matrix too large");
    if (device < 0 || device >= kDtwMaxDevices) return fail(WLK_ERR_ARG, "dtw: device out of range");
    return guarded([&]() {
        WLK_HIP(hipSetDevice(device));
        const size_t nx = (size_t)n_rows * n_cols, nt = (size_t)(n_rows + 1) * (n_cols + 1);
        DtwWorkspace& ws = g_dtw_ws[device];
        std::lock_guard<std::mutex> lk(ws.mu);
        ws.reserve(nx, nt);
        std::memcpy(ws.pinned, x, nx * sizeof(float));
        WLK_HIP(hipMemcpyAsync(ws.xd, ws.pinned, nx * sizeof(float), hipMemcpyHostToDevice, ws.stream));
        launch_dtw(ws.stream, ws.xd, n_rows, n_cols, ws.td, ws.tt);
        // (the upload has been consumed by the time the kernels are done: the pinned block is reused for the way back)
        WLK_HIP(hipMemcpyAsync(ws.pinned, ws.tt, nt, hipMemcpyDeviceToHost, ws.stream));
        WLK_HIP(hipStreamSynchronize(ws.stream));
        std::memcpy(trace, ws.pinned, nt);
        return WLK_OK;
    });
}

// Tests: the production ragged launches (recurrence, transposition, path walk) on host-given cost matrices; no model.
extern "C" int wlk_diag_dtw_starts(const float* costs, const int64_t* offsets, const int32_t* n_rows, const int32_t* n_cols, int n,
                                   int32_t* starts, int8_t* traces) {
    if (!costs || !offsets || !n_rows || !n_cols || !starts) return fail(WLK_ERR_ARG, "dtw starts: NULL argument");
    if (n < 1 || n > kAlignWinMax) return fail(WLK_ERR_ARG, "dtw starts: 1..8 matrices");
    size_t n_x = 0, n_t = 0, n_s = 0;
    for (int i = 0; i < n; ++i) {
        if (n_rows[i] < 1 || n_rows[i] > kDtwMaxRows || n_cols[i] < 1 || n_cols[i] > kDtwWalkMaxCols || offsets[i] < 0)
            return fail(WLK_ERR_ARG, "dtw starts: 1..1024 rows, 1..4095 columns, offsets >= 0");
        n_x = std::max(n_x, (size_t)offsets[i] + (size_t)n_rows[i] * n_cols[i]);
        n_t += (size_t)(n_rows[i] + 1) * (n_cols[i] + 1);
        n_s += (size_t)n_rows[i];
    }
    return guarded([&]() {
        struct Scratch {
            hipStream_t stream = nullptr;
            float* x = nullptr;
            signed char *tt = nullptr, *tr = nullptr;
            int* st = nullptr;
            AlignWin* tab = nullptr;
            ~Scratch() {
                for (void* p : {(void*)x, (void*)tt, (void*)tr, (void*)st, (void*)tab})
                    if (p) (void)hipFree(p);
                if (stream) (void)hipStreamDestroy(stream);
            }
        } w;
        WLK_HIP(hipStreamCreateWithFlags(&w.stream, hipStreamNonBlocking));
        WLK_HIP(hipMalloc(reinterpret_cast<void**>(&w.x), n_x * sizeof(float)));
        WLK_HIP(hipMalloc(reinterpret_cast<void**>(&w.tt), n_t));
        WLK_HIP(hipMalloc(reinterpret_cast<void**>(&w.tr), n_t));
        WLK_HIP(hipMalloc(reinterpret_cast<void**>(&w.st), n_s * sizeof(int)));
        WLK_HIP(hipMalloc(reinterpret_cast<void**>(&w.tab), sizeof(AlignWin) * kAlignWinMax));
        AlignWin host[kAlignWinMax] = {};
        size_t at_t = 0, at_s = 0;
        for (int i = 0; i < n; ++i) {
            AlignWin& t = host[i];
            t.cost = w.x + offsets[i];
            t.trace_t = w.tt + at_t;
            t.trace = w.tr + at_t;
            t.starts = w.st + at_s;
            t.N = n_rows[i];
            t.F = n_cols[i];
            at_t += (size_t)(n_rows[i] + 1) * (n_cols[i] + 1);
            at_s += (size_t)n_rows[i];
        }
        WLK_HIP(hipMemcpy(w.x, costs, n_x * sizeof(float), hipMemcpyHostToDevice));
        WLK_HIP(hipMemcpy(w.tab, host, sizeof(AlignWin) * n, hipMemcpyHostToDevice));
        WLK_HIP(hipMemsetAsync(w.tt, 0xff, n_t, w.stream));   // -1 like dtw_cpu's untouched border cells
        launch_dtw_ragged(LaunchCtx{w.stream, nullptr}, w.tab, host, n);
        WLK_HIP(hipStreamSynchronize(w.stream));
        WLK_HIP(hipMemcpy(starts, w.st, n_s * sizeof(int), hipMemcpyDeviceToHost));
        if (traces) WLK_HIP(hipMemcpy(traces, w.tr, n_t, hipMemcpyDeviceToHost));
        return WLK_OK;
    });
}
