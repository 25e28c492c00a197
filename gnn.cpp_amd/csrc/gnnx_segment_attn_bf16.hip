// Dense segment attention on bf16 operands (include/gnnx.h "dense segment attention, bf16 operands"): gnnx_segment_attn.hip's three calls with
// Q, K, V and G stored as bf16, every product on v_mfma_f32_32x32x16_bf16, f32 accumulation, f32 statistics and f32 outputs.  The
// definitions (s, m, x, z, Y, dot, alpha, ds, dQ, dK, dV), the WORK SPLIT (one wavefront per 32-row tile of the whole batch x head,
// first_segment / for_segments, masked rows never loaded, one accumulator per output element) are that file's.  What differs:
//
// MATRIX INSTRUCTION (D[m][n] += A[m][k] B[k][n], k = 0 .. 15): lane l gives A[l & 31][8 (l >> 5) + j] and B[8 (l >> 5) + j][l & 31],
// j = 0 .. 7, as eight packed bf16 (one 16-byte register group each) and holds D[rowof(r, l >> 5)][l & 31] in register r -- the f32
// kernels' accumulator layout.  A product of two bf16 is exact in f32; the sums are the matrix pipe's.
//
// OPERAND IMAGES IN LDS, both bf16, built by one copy-in from one global load.
//   ROW image [32][DP + 8]: streamed row r, feature d at r (DP + 8) + d.  It feeds the score-like products S^T = K Q^T, dP^T = V G^T
//     (column side S = Q K^T, dP = G V^T): lane l reads ONE 16-byte piece of row l & 31 at feature 16 c + 8 (l >> 5) per MFMA.  The
//     pitch is (DP + 8) / 8 = 3, 5, 9 or 17 sixteen-byte units, an odd count: LDS serves a 16-byte read in groups of lanes, and the
//     consecutive rows of a group start 1 unit (mod 2), hence 4 banks (mod 8), apart until the 64 banks are covered -- with the pitch
//     DP itself every row would start on bank 0.  The own tile (Q; Q and G; K and V) goes through the same image once and then stays
//     in registers as DP / 16 packed B operands (4 dwords each; DP / 2 floats in the f32 kernels).
//   TRANSPOSED image [DP][32 + 8]: feature d, slot p at d * 40 + p.  It feeds the output-like products O^T += V^T P^T, dQ^T += K^T dS^T,
//     dV^T += G^T alpha, dK^T += Q^T dS, whose k runs over STREAMED ROWS, 16 per k-step s.  The B operand of k-step s is registers
//     8 s .. 8 s + 7 of the weight tile in the accumulator layout, rounded to bf16 and packed in place: slot j of half-wave hf is
//     streamed row rowof(8 s + j, hf) = 16 s + 8 (j >> 2) + 4 hf + (j & 3).  So the image stores streamed row R at slot
//     slot_of(R) = R with bits 2 and 3 exchanged ( = 16 s + 8 hf + j), and lane l's A operand of k-step s is ONE 16-byte read of line
//     32 i + (l & 31) at slot 16 s + 8 (l >> 5).  The weights never go to LDS.  Pitch 40 = 5 sixteen-byte units, odd as above.
//   WHY SCATTER, not ds_read_b64_tr_b16 on a row image: the transpose read returns the hardware's fixed 4 x 4 arrangement of 8-byte
//     pieces, so the row permutation above would have to be made in the row image (breaking its 16-byte score-like reads of whole
//     rows) or by a second exchange of the weights; and an A operand would be two 8-byte reads.  The scatter gets the permutation for
//     free (it is an address), keeps every operand read one aligned 16-byte read, and is plain C++.  Its cost is eight 2-byte LDS stores
//     per 16-byte piece; a copy-in that builds a transposed image deals lanes ROW-fastest (lane -> row e % 32) so that the 32 lanes
//     of one store fall on 16 consecutive dwords of one line (two lanes share a dword, the two 8-feature pieces of a pass lie
//     8 * 80 bytes = 32 banks apart); a copy-in that builds only a row image deals them feature-fastest (full global lines).
//   Built per kernel, only what is read:  forward K row, V transposed;  row side K both, V row;  column side Q both, G both.
//   LDS bytes (DP = 16 / 32 / 64 / 128): row image 1 536 / 2 560 / 4 608 / 8 704, transposed image 1 280 / 2 560 / 5 120 / 10 240;
//     forward 2 816 / 5 120 / 9 728 / 18 944, row side 4 352 / 7 680 / 14 336 / 27 648, column side 6 016 / 10 624 / 19 840 / 38 272
//     (with 384 bytes of statistics).
//
// COPY-IN.  16-byte global loads (8 bf16) where D % 8 == 0 and every bf16 pointer and pitch is 16-byte aligned (ld % 8 == 0), 2-byte
// loads into the SAME images otherwise; the f32 side (Y, dQ, dK, dV, the row side's Y input) keeps store_own's float4 / scalar choice
// independently.  Rows at or past the segment's end and features past D are zeros in both images.
//
// ORDER.  The dot products and the sums over a tile's 32 rows run in v_mfma_f32_32x32x16_bf16 (exact products, f32 accumulation, the
// hardware's internal order).  Outside it every operation is ONE separately rounded fp32 operation, in the f32 kernels' order:  s takes
// one multiply by scale;  per streamed tile m' = max(m, the tile's maximum),  r = 1 if m == m' else expf(m - m'),  x = expf(s - m'),
// the tile's sum = (the lane's 16 x ascending) + (the other half-wave's), taken from the UNROUNDED x,  z = z * r + that,  N = N * r,
// then x is the operand that accumulates onto N;  Y = N / z is one IEEE division.  rowmax = m is the maximum of scale * s and
// rowsum = z.  Backward:  alpha = expf(scale * s - m) / z (one expf, one division), ds = alpha * (dP - dot) in f32;  alpha is the dV
// operand and ds the dQ / dK operand;  the accumulators start from +0, dQ and dK take one multiply by scale, beta = 1 is one add of
// the old value.  dot = <G, Y>: the lane's DP / 2 products float(G) * Y (f32, each rounded) added ascending from +0, plus the other
// half-wave's.
// A WEIGHT OPERAND (x, alpha, ds -- these three and nothing else) enters the matrix pipe as TWO bf16 terms, hi = bf16(w) rounded to
// nearest even and lo = bf16(w - hi) of the exact remainder, one MFMA each, hi first.  |w - hi| <= 2^-8 |w| (half of bf16's spacing
// 2^-7 just above a power of two) and lo carries that remainder to another 2^-8, so the operand is w to 2^-16 relative.  hi alone
// cannot meet a bar that allows 2^-9 per operand (tests/segment_attn_bf16_ref.py): it misses it whenever the few alpha of a sum lie
// just above a power of two.  The second term costs one more MFMA per output-like k-step (at D = 128: 8 + 16 matrix instructions a
// forward tile, 16 + 16 row side, 16 + 32 column side, against 64 + 64, 128 + 64, 128 + 128 in f32).
// Every loop is bounded by n_seg or by a segment length clipped to [0, n_rows].
#include "gnnx_segment_tiles.h"   // rowof, rescale_of, first_segment, for_segments, store_own, the status checks

#pragma clang fp contract(off)

using namespace gnnx;
using namespace gnnx::seg;

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kTrPitch = kTile + 8;   // slots of a transposed line

template <int DP> struct Img {
    static constexpr int kRowPitch = DP + 8;
    static constexpr int kRow = kTile * kRowPitch;   // bf16 elements of a row image
    static constexpr int kTr = DP * kTrPitch;        // of a transposed image
};

struct Args {
    int32_t n_seg, n_rows, H, D;
    const int32_t *segptr;
    float scale;
    const uint16_t *Q, *K, *V, *G;
    const float *Yin;
    int64_t ldq, ldk, ldv, ldg, ldyin;
    const float *rowmax, *rowsum, *dot;        // backward inputs, [n_rows, H] (dot: column side)
    float *rowmax_out, *rowsum_out, *dot_out;  // forward outputs; row side: dot
    float *A, *B;                              // forward: Y; row side: dQ; column side: dV, dK
    int64_t lda, ldb;
    int beta;
};

// the slot of streamed row R in a transposed line: bits 2 and 3 exchanged
__device__ __forceinline__ int slot_of(int R) { return (R & 19) | ((R & 4) << 1) | ((R & 8) >> 1); }

// rows [row0, row0 + 32) of M's columns col0 .. col0 + D - 1 -> the row image (ROW) and / or the transposed image (TR); rows at or past
// row_end and columns past D are zeros
template <int DP, bool VEC, bool ROW, bool TR>
__device__ __forceinline__ void copy_in(uint16_t *rows, uint16_t *tr, const uint16_t *M, int64_t ld, int64_t col0, int32_t D, int64_t row0,
                                        int64_t row_end, int lane)
{
    constexpr int LD = Img<DP>::kRowPitch;
    if constexpr (VEC) {
        constexpr int CH = DP / 8;
#pragma unroll
        for (int e0 = 0; e0 < kTile * CH; e0 += kWave) {
            const int e = e0 + lane;
            const int r = TR ? e % kTile : e / CH, c = TR ? e / kTile : e % CH;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (row0 + r < row_end && 8 * c < D) v = *reinterpret_cast<const uint4 *>(M + (row0 + r) * ld + col0 + 8 * c);
            if constexpr (ROW) *reinterpret_cast<uint4 *>(rows + r * LD + 8 * c) = v;
            if constexpr (TR) {
                uint16_t *p = tr + 8 * c * kTrPitch + slot_of(r);
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    p[(2 * k) * kTrPitch] = (uint16_t)(w[k] & 0xffffu);
                    p[(2 * k + 1) * kTrPitch] = (uint16_t)(w[k] >> 16);
                }
            }
        }
    } else {
#pragma unroll 8
        for (int e0 = 0; e0 < kTile * DP; e0 += kWave) {
            const int e = e0 + lane;
            const int r = TR ? e % kTile : e / DP, c = TR ? e / kTile : e % DP;
            const uint16_t v = (row0 + r < row_end && c < D) ? M[(row0 + r) * ld + col0 + c] : (uint16_t)0;
            if constexpr (ROW) rows[r * LD + c] = v;
            if constexpr (TR) tr[c * kTrPitch + slot_of(r)] = v;
        }
    }
}

// the lane's B operands of the score-like products: b[c] = rows[l & 31][16 c + 8 (l >> 5) .. + 7]
template <int DP>
__device__ __forceinline__ void own_regs(const uint16_t *rows, bf16x8 (&b)[DP / 16], int lane)
{
    const uint16_t *p = rows + (lane & 31) * Img<DP>::kRowPitch + 8 * (lane >> 5);
#pragma unroll
    for (int c = 0; c < DP / 16; c++) b[c] = *reinterpret_cast<const bf16x8 *>(p + 16 * c);
}

// acc[rowof(r, hf)][l & 31] = sum_d rows[rowof(r, hf)][d] * own[l & 31][d]
template <int DP>
__device__ __forceinline__ f32x16 score_like(const uint16_t *rows, const bf16x8 (&b)[DP / 16], int lane)
{
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = 0.f;
    const uint16_t *p = rows + (lane & 31) * Img<DP>::kRowPitch + 8 * (lane >> 5);
#pragma unroll
    for (int c = 0; c < DP / 16; c++)
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8 *>(p + 16 * c), b[c], acc, 0, 0, 0);
    return acc;
}

// out[i][rowof(r, hf)] (feature 32 i + rowof) [l & 31] += sum over the 32 streamed rows of tr[feature][slot] * (hi + lo)(w) of the lane
// that owns [l & 31]: registers 8 s .. 8 s + 7 of w are k-step s's B operand, as TWO packed bf16 terms -- hi = bf16(w), to nearest
// even, and lo = bf16(w - hi) of the exact f32 remainder -- accumulated hi first
template <int DP>
__device__ __forceinline__ void out_like(const uint16_t *tr, const f32x16 &w, f32x16 (&out)[blocks_of<DP>()], int lane)
{
    const int col = lane & 31, hf = lane >> 5;
#pragma unroll
    for (int s = 0; s < 2; s++) {
        bf16x8 b, b_lo;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const float x = w[8 * s + j];
            const __bf16 h = (__bf16)x;
            b[j] = h;
            b_lo[j] = (__bf16)(x - (float)h);   // |x - h| <= 2^-8 |x| and on x's grid: the subtraction is exact
        }
#pragma unroll
        for (int i = 0; i < blocks_of<DP>(); i++) {
            bf16x8 av;
            if constexpr (DP < 32) {   // the MFMA's rows past the padded head width
#pragma unroll
                for (int j = 0; j < 8; j++) av[j] = (__bf16)0.f;
                if (col < DP) av = *reinterpret_cast<const bf16x8 *>(tr + col * kTrPitch + 16 * s + 8 * hf);
            } else {
                av = *reinterpret_cast<const bf16x8 *>(tr + (32 * i + col) * kTrPitch + 16 * s + 8 * hf);
            }
            out[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, b, out[i], 0, 0, 0);
            out[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, b_lo, out[i], 0, 0, 0);
        }
    }
}

template <int DP>
__device__ __forceinline__ void clear(f32x16 (&acc)[blocks_of<DP>()])
{
#pragma unroll
    for (int i = 0; i < blocks_of<DP>(); i++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[i][r] = 0.f;
}

// ---- forward -----------------------------------------------------------------------------------------------------------------------
template <int DP, bool VIN, bool VOUT>
__global__ __launch_bounds__(kWave) void fwd_kernel(Args a)
{
    __shared__ __attribute__((aligned(16))) uint16_t ks[Img<DP>::kRow], vt[Img<DP>::kTr];
    const int lane = threadIdx.x, hf = lane >> 5;
    const int64_t r0 = (int64_t)blockIdx.x * kTile, r1 = r0 + kTile < a.n_rows ? r0 + kTile : a.n_rows;
    const int64_t row = r0 + (lane & 31);
    const int32_t h = blockIdx.y;
    const int64_t c0 = (int64_t)h * a.D;

    copy_in<DP, VIN, true, false>(ks, nullptr, a.Q, a.ldq, c0, a.D, r0, r1, lane);
    __syncthreads();
    bf16x8 q[DP / 16];
    own_regs<DP>(ks, q, lane);
    __syncthreads();

    f32x16 N[blocks_of<DP>()];
    clear<DP>(N);
    float m = -INFINITY, z = 0.f;

    for_segments(a.segptr, a.n_seg, a.n_rows, r0, r1, row, [&](int64_t lo, int64_t hi, bool active) {
        for (int64_t kb = lo; kb < hi; kb += kTile) {
            copy_in<DP, VIN, true, false>(ks, nullptr, a.K, a.ldk, c0, a.D, kb, hi, lane);
            copy_in<DP, VIN, false, true>(nullptr, vt, a.V, a.ldv, c0, a.D, kb, hi, lane);
            __syncthreads();
            f32x16 s = score_like<DP>(ks, q, lane);
            float tmax = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                s[r] = (active && kb + rowof(r, hf) < hi) ? a.scale * s[r] : -INFINITY;
                tmax = fmaxf(tmax, s[r]);
            }
            tmax = fmaxf(tmax, __shfl_xor(tmax, 32, kWave));
            const float m_new = active ? fmaxf(m, tmax) : m;
            const float rs = active ? rescale_of(m, m_new) : 1.f;
            float zt = 0.f;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                s[r] = active ? expf(s[r] - m_new) : 0.f;   // a masked key: expf(-inf) = +0
                zt = zt + s[r];
            }
            zt = zt + __shfl_xor(zt, 32, kWave);
            z = z * rs + zt;
            m = m_new;
#pragma unroll
            for (int i = 0; i < blocks_of<DP>(); i++)
#pragma unroll
                for (int r = 0; r < 16; r++) N[i][r] = N[i][r] * rs;
            out_like<DP>(vt, s, N, lane);
            __syncthreads();
        }
    });

    if (row >= r1) return;
    const bool some = z > 0.f;   // a row that no segment holds: Y = +0, m = -inf, z = +0
    store_own<DP, VOUT>(N, a.A, a.lda, row, c0, a.D, lane, [&](float n, const float *) { return some ? __fdiv_rn(n, z) : 0.f; });
    if (hf == 0) {
        a.rowmax_out[row * a.H + h] = m;
        a.rowsum_out[row * a.H + h] = z;
    }
}

// ---- backward, row side ----------------------------------------------------------------------------------------------------------
template <int DP, bool VIN, bool VOUT>
__global__ __launch_bounds__(kWave) void bwd_rows_kernel(Args a)
{
    __shared__ __attribute__((aligned(16))) uint16_t ks[Img<DP>::kRow], vs[Img<DP>::kRow], kt[Img<DP>::kTr];
    const int lane = threadIdx.x, hf = lane >> 5;
    const int64_t r0 = (int64_t)blockIdx.x * kTile, r1 = r0 + kTile < a.n_rows ? r0 + kTile : a.n_rows;
    const int64_t row = r0 + (lane & 31);
    const int32_t h = blockIdx.y;
    const int64_t c0 = (int64_t)h * a.D;

    copy_in<DP, VIN, true, false>(ks, nullptr, a.Q, a.ldq, c0, a.D, r0, r1, lane);
    copy_in<DP, VIN, true, false>(vs, nullptr, a.G, a.ldg, c0, a.D, r0, r1, lane);
    __syncthreads();
    bf16x8 q[DP / 16], g[DP / 16];
    own_regs<DP>(ks, q, lane);
    own_regs<DP>(vs, g, lane);
    __syncthreads();

    const bool mine = row < r1;
    float dot = 0.f;
    if (mine) {   // the lane's features of its own row of Y, straight from global memory: read once
        const float *y = a.Yin + row * a.ldyin + c0;
#pragma unroll
        for (int c = 0; c < DP / 16; c++)
#pragma unroll
            for (int p = 0; p < 2; p++) {
                const int d = 16 * c + 8 * hf + 4 * p;
                float yv[4] = {0.f, 0.f, 0.f, 0.f};
                if constexpr (VOUT) {
                    if (d < a.D) {
                        const float4 t = *reinterpret_cast<const float4 *>(y + d);
                        yv[0] = t.x, yv[1] = t.y, yv[2] = t.z, yv[3] = t.w;
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 4; j++)
                        if (d + j < a.D) yv[j] = y[d + j];
                }
#pragma unroll
                for (int j = 0; j < 4; j++) dot = dot + (float)g[c][4 * p + j] * yv[j];
            }
    }
    dot = dot + __shfl_xor(dot, 32, kWave);
    if (mine && hf == 0) a.dot_out[row * a.H + h] = dot;
    const float m = mine ? a.rowmax[row * a.H + h] : 0.f, z = mine ? a.rowsum[row * a.H + h] : 1.f;

    f32x16 dq[blocks_of<DP>()];
    clear<DP>(dq);

    for_segments(a.segptr, a.n_seg, a.n_rows, r0, r1, row, [&](int64_t lo, int64_t hi, bool active) {
        for (int64_t kb = lo; kb < hi; kb += kTile) {
            copy_in<DP, VIN, true, true>(ks, kt, a.K, a.ldk, c0, a.D, kb, hi, lane);
            copy_in<DP, VIN, true, false>(vs, nullptr, a.V, a.ldv, c0, a.D, kb, hi, lane);
            __syncthreads();
            f32x16 s = score_like<DP>(ks, q, lane);
            const f32x16 dp = score_like<DP>(vs, g, lane);
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const bool valid = active && kb + rowof(r, hf) < hi;
                const float al = __fdiv_rn(expf(a.scale * s[r] - m), z);
                s[r] = valid ? al * (dp[r] - dot) : 0.f;
            }
            out_like<DP>(kt, s, dq, lane);
            __syncthreads();
        }
    });

    if (!mine) return;
    store_own<DP, VOUT>(dq, a.A, a.lda, row, c0, a.D, lane, [&](float v, const float *) { return a.scale * v; });
}

// ---- backward, column side ---------------------------------------------------------------------------------------------------------
template <int DP, bool VIN, bool VOUT>
__global__ __launch_bounds__(kWave) void bwd_cols_kernel(Args a)
{
    __shared__ __attribute__((aligned(16))) uint16_t qs[Img<DP>::kRow], gs[Img<DP>::kRow], qt[Img<DP>::kTr], gt[Img<DP>::kTr];
    __shared__ float st_m[kTile], st_z[kTile], st_d[kTile];
    const int lane = threadIdx.x, hf = lane >> 5;
    const int64_t r0 = (int64_t)blockIdx.x * kTile, r1 = r0 + kTile < a.n_rows ? r0 + kTile : a.n_rows;
    const int64_t row = r0 + (lane & 31);   // the lane's own KEY
    const int32_t h = blockIdx.y;
    const int64_t c0 = (int64_t)h * a.D;

    copy_in<DP, VIN, true, false>(qs, nullptr, a.K, a.ldk, c0, a.D, r0, r1, lane);
    copy_in<DP, VIN, true, false>(gs, nullptr, a.V, a.ldv, c0, a.D, r0, r1, lane);
    __syncthreads();
    bf16x8 k[DP / 16], v[DP / 16];
    own_regs<DP>(qs, k, lane);
    own_regs<DP>(gs, v, lane);
    __syncthreads();

    f32x16 dv[blocks_of<DP>()], dk[blocks_of<DP>()];
    clear<DP>(dv);
    clear<DP>(dk);

    for_segments(a.segptr, a.n_seg, a.n_rows, r0, r1, row, [&](int64_t lo, int64_t hi, bool active) {
        for (int64_t qb = lo; qb < hi; qb += kTile) {
            copy_in<DP, VIN, true, true>(qs, qt, a.Q, a.ldq, c0, a.D, qb, hi, lane);
            copy_in<DP, VIN, true, true>(gs, gt, a.G, a.ldg, c0, a.D, qb, hi, lane);
            if (lane < kTile) {   // a query past the segment's end: finite statistics, its weight is masked below
                const int64_t i = qb + lane;
                const bool ok = i < hi;
                st_m[lane] = ok ? a.rowmax[i * a.H + h] : 0.f;
                st_z[lane] = ok ? a.rowsum[i * a.H + h] : 1.f;
                st_d[lane] = ok ? a.dot[i * a.H + h] : 0.f;
            }
            __syncthreads();
            f32x16 al = score_like<DP>(qs, k, lane);
            f32x16 ds = score_like<DP>(gs, v, lane);
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int i = rowof(r, hf);
                const bool valid = active && qb + i < hi;
                const float w = __fdiv_rn(expf(a.scale * al[r] - st_m[i]), st_z[i]);
                al[r] = valid ? w : 0.f;
                ds[r] = valid ? w * (ds[r] - st_d[i]) : 0.f;
            }
            out_like<DP>(gt, al, dv, lane);
            out_like<DP>(qt, ds, dk, lane);
            __syncthreads();
        }
    });

    if (row >= r1) return;
    const bool add = a.beta != 0;
    store_own<DP, VOUT>(dv, a.A, a.lda, row, c0, a.D, lane, [&](float x, const float *old) { return add ? *old + x : x; });
    store_own<DP, VOUT>(dk, a.B, a.ldb, row, c0, a.D, lane, [&](float x, const float *old) {
        const float t = a.scale * x;
        return add ? *old + t : t;
    });
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
inline bool vec8(int64_t ld, const void *p) { return ld % 8 == 0 && aligned16(p); }   // 8 bf16 may be loaded from any row of p

#define SEG_ATTN_ONE(kernel, DP)                                                                                   \
    do {                                                                                                           \
        if (vin && vout) hipLaunchKernelGGL((kernel<DP, true, true>), grid, dim3(kWave), 0, st, a);                \
        else if (vin) hipLaunchKernelGGL((kernel<DP, true, false>), grid, dim3(kWave), 0, st, a);                  \
        else if (vout) hipLaunchKernelGGL((kernel<DP, false, true>), grid, dim3(kWave), 0, st, a);                 \
        else hipLaunchKernelGGL((kernel<DP, false, false>), grid, dim3(kWave), 0, st, a);                          \
    } while (0)

// the instantiation whose padded width holds D, on the 16-byte or the scalar path of the bf16 inputs (vin) and of the f32 side (vout)
#define SEG_ATTN_LAUNCH(kernel)                                                                        \
    do {                                                                                               \
        const dim3 grid((uint32_t)ceil_div(a.n_rows, kTile), (uint32_t)a.H);                           \
        hipStream_t st = as_stream(stream);                                                            \
        GNNX_SEG_FOR_DP(a.D, SEG_ATTN_ONE, kernel);                                                    \
        GNNX_LAUNCH_CHECK();                                                                           \
    } while (0)

}  // namespace

GNNX_API int gnnx_segment_attn_bf16_f32(int32_t n_seg, int32_t n_rows, const int32_t *d_segptr, int32_t n_heads, int32_t head_dim, float scale,
                                        const uint16_t *d_Q, int64_t ldq, const uint16_t *d_K, int64_t ldk, const uint16_t *d_V, int64_t ldv,
                                        float *d_Y, int64_t ldy, float *d_rowmax, float *d_rowsum, void *stream)
{
    const int rc = check_self_attn(n_seg, n_rows, n_heads, head_dim);
    if (rc) return rc;
    const int64_t F = (int64_t)n_heads * head_dim;
    GNNX_REQUIRE(ldq >= F && ldk >= F && ldv >= F && ldy >= F, GNNX_ERR_INVALID_ARG, "ld < n_heads * head_dim");
    if (n_rows == 0 || n_seg == 0) return GNNX_OK;
    GNNX_REQUIRE(d_segptr && d_Q && d_K && d_V && d_Y && d_rowmax && d_rowsum, GNNX_ERR_INVALID_ARG, "null pointer");
    Args a{};
    a.n_seg = n_seg, a.n_rows = n_rows, a.H = n_heads, a.D = head_dim, a.segptr = d_segptr, a.scale = scale;
    a.Q = d_Q, a.ldq = ldq, a.K = d_K, a.ldk = ldk, a.V = d_V, a.ldv = ldv, a.A = d_Y, a.lda = ldy, a.rowmax_out = d_rowmax, a.rowsum_out = d_rowsum;
    const bool vin = head_dim % 8 == 0 && vec8(ldq, d_Q) && vec8(ldk, d_K) && vec8(ldv, d_V);
    const bool vout = head_dim % 4 == 0 && vec4(ldy, d_Y);
    SEG_ATTN_LAUNCH(fwd_kernel);
    return GNNX_OK;
}

GNNX_API int gnnx_segment_attn_bwd_rows_bf16_f32(int32_t n_seg, int32_t n_rows, const int32_t *d_segptr, int32_t n_heads, int32_t head_dim,
                                                 float scale, const uint16_t *d_G, int64_t ldg, const uint16_t *d_Q, int64_t ldq,
                                                 const uint16_t *d_K, int64_t ldk, const uint16_t *d_V, int64_t ldv, const float *d_Y, int64_t ldy,
                                                 const float *d_rowmax, const float *d_rowsum, float *d_dQ, int64_t lddq, float *d_dot,
                                                 void *stream)
{
    const int rc = check_self_attn(n_seg, n_rows, n_heads, head_dim);
    if (rc) return rc;
    const int64_t F = (int64_t)n_heads * head_dim;
    GNNX_REQUIRE(ldg >= F && ldq >= F && ldk >= F && ldv >= F && ldy >= F && lddq >= F, GNNX_ERR_INVALID_ARG, "ld < n_heads * head_dim");
    if (n_rows == 0 || n_seg == 0) return GNNX_OK;
    GNNX_REQUIRE(d_segptr && d_G && d_Q && d_K && d_V && d_Y && d_rowmax && d_rowsum && d_dQ && d_dot, GNNX_ERR_INVALID_ARG, "null pointer");
    Args a{};
    a.n_seg = n_seg, a.n_rows = n_rows, a.H = n_heads, a.D = head_dim, a.segptr = d_segptr, a.scale = scale;
    a.G = d_G, a.ldg = ldg, a.Q = d_Q, a.ldq = ldq, a.K = d_K, a.ldk = ldk, a.V = d_V, a.ldv = ldv, a.Yin = d_Y, a.ldyin = ldy;
    a.rowmax = d_rowmax, a.rowsum = d_rowsum, a.A = d_dQ, a.lda = lddq, a.dot_out = d_dot;
    const bool vin = head_dim % 8 == 0 && vec8(ldg, d_G) && vec8(ldq, d_Q) && vec8(ldk, d_K) && vec8(ldv, d_V);
    const bool vout = head_dim % 4 == 0 && vec4(ldy, d_Y) && vec4(lddq, d_dQ);
    SEG_ATTN_LAUNCH(bwd_rows_kernel);
    return GNNX_OK;
}

GNNX_API int gnnx_segment_attn_bwd_cols_bf16_f32(int32_t n_seg, int32_t n_rows, const int32_t *d_segptr, int32_t n_heads, int32_t head_dim,
                                                 float scale, const uint16_t *d_G, int64_t ldg, const uint16_t *d_Q, int64_t ldq,
                                                 const uint16_t *d_K, int64_t ldk, const uint16_t *d_V, int64_t ldv, const float *d_rowmax,
                                                 const float *d_rowsum, const float *d_dot, float beta, float *d_dK, int64_t lddk, float *d_dV,
                                                 int64_t lddv, void *stream)
{
    const int rc = check_self_attn(n_seg, n_rows, n_heads, head_dim);
    if (rc) return rc;
    const int64_t F = (int64_t)n_heads * head_dim;
    GNNX_REQUIRE(ldg >= F && ldq >= F && ldk >= F && ldv >= F && lddk >= F && lddv >= F, GNNX_ERR_INVALID_ARG, "ld < n_heads * head_dim");
    GNNX_REQUIRE(beta == 0.f || beta == 1.f, GNNX_ERR_INVALID_ARG, "beta must be 0 or 1");
    if (n_rows == 0 || n_seg == 0) return GNNX_OK;
    GNNX_REQUIRE(d_segptr && d_G && d_Q && d_K && d_V && d_rowmax && d_rowsum && d_dot && d_dK && d_dV, GNNX_ERR_INVALID_ARG, "null pointer");
    Args a{};
    a.n_seg = n_seg, a.n_rows = n_rows, a.H = n_heads, a.D = head_dim, a.segptr = d_segptr, a.scale = scale;
    a.G = d_G, a.ldg = ldg, a.Q = d_Q, a.ldq = ldq, a.K = d_K, a.ldk = ldk, a.V = d_V, a.ldv = ldv;
    a.rowmax = d_rowmax, a.rowsum = d_rowsum, a.dot = d_dot, a.A = d_dV, a.lda = lddv, a.B = d_dK, a.ldb = lddk, a.beta = beta != 0.f;
    const bool vin = head_dim % 8 == 0 && vec8(ldg, d_G) && vec8(ldq, d_Q) && vec8(ldk, d_K) && vec8(ldv, d_V);
    const bool vout = head_dim % 4 == 0 && vec4(lddk, d_dK) && vec4(lddv, d_dV);
    SEG_ATTN_LAUNCH(bwd_cols_kernel);
    return GNNX_OK;
}
