// k_tonebank.hip -- per-row tone detector and tone squelch over the rows of a
// bank (ToneBank): for every block of B samples of every row of a float32
// [C][n] image, the power at F tones common to all rows, the dominant tone and
// a gate that holds.  The definition is the project's own (include/ldsp.h):
//   Xre[k] = sum_i Tc[k][i] x[c][bB + i],  Xim[k] = sum_i Ts[k][i] x[c][bB + i]
//   power[c][b][k] = fmaf(Xre, Xre, Xim * Xim)
//   tone[c][b] = the dominant tone or -1;  open[c][b]: a block in [b - hold, b]
//   was accepted;  y = open ? x : +0
// A row's stream in a call is its `fill` carried samples (the object's history
// buffer) followed by the call's n, as in k_sqbank.hip.  Three plain launches,
// no workgroup waits on another:
//
// k_tonebank_power: the matrix product [P x B] . [B x columns] on
//   v_mfma_f32_32x32x2_f32.  A column is one (row, block) pair of the call,
//   column = row * nblocks + block; the P = 32 M matrix rows are the table rows
//   (cosine and sine of 16 tones per 32, zero rows after the last tone).  A wave
//   owns 32 columns and keeps all M <= 4 row tiles of them in accumulators: lane
//   l loads the four samples 8q + 4 (l >> 5) .. + 3 of column l & 31 with one
//   16-byte load, and the four table values of the same samples for matrix row
//   l & 31 of each tile with one 16-byte load from a table laid out for exactly
//   that (tonebank_pack); MFMA u of a group of four then multiplies samples
//   8q + u (k = 0) and 8q + 4 + u (k = 1), so an accumulator element is the
//   fmaf chain over its samples in the order 0 4 1 5 2 6 3 7 8 12 9 13 ..
//   The chain is cut into segments of tb_seg(B) samples, about 2 sqrt(B) (the
//   last one shorter), each from +0, and the segment sums are added in float64
//   in segment order and rounded once to float32: the rounding error of one
//   float32 chain grows with the root of its length (measured 1.2e-6 of the
//   row's scale for one chain of 192 samples, 2.4e-6 of the largest power
//   emulated for 4096), and a float32 sum of the segment sums would grow the
//   same way with their number; with S^2 / B = 4 the chains' errors stay near
//   two roundings whatever B is.  From B = kTbSplitB up the four waves of a
//   workgroup share one column tile, each with a quarter of the segments, and
//   wave 0 adds the four float64 sums in wave order; below, each wave has a
//   column tile of its own.  Both rules depend on B alone, so a block's bits do
//   not depend on the tile, the call or C.
//   The accumulator layout puts matrix rows (reg & 3) + 8 (reg >> 2) + 4 (l >> 5)
//   on lane l; the table's row order (tb_row) puts a tone's cosine in register
//   r and its sine in register r + 4 of the same lane, so the power needs no
//   lane movement.  Workgroups after the column tiles write the rows' next
//   carry into the other buffer of the pair.
// k_tonebank_detect: one lane per (row, block): the largest power, the
//   dominance test in float64, the accepted flag; a workgroup takes kTbDetTile
//   blocks of a row and recomputes the flags of the kTbHalo blocks before them,
//   so the hold window is a look-back over flags in LDS; blocks before the call
//   are stood for by the carried counter (blocks since the last accepted one).
//   The row's last workgroup writes the next counter into the other buffer.
// k_tonebank_gate (not launched for a measurement): 16 bytes per lane; closed
//   blocks are written as zeros without being read.
#include "kernels.hpp"
#include "ldsp_common.hpp"

namespace ldsp {
namespace k {

namespace {

constexpr int kTbThreads = 256;
constexpr int kTbSplitB = 4096;               // from here up a workgroup's four waves share a column tile
constexpr int kTbHalo = 64;                   // = kTonebankMaxHold: blocks of look-back a detect workgroup recomputes
constexpr int kTbDetTile = kTbThreads - kTbHalo;
constexpr int kTbGateTile = 8192;             // samples per workgroup of the gate

typedef float TbAcc __attribute__((ext_vector_type(16)));
typedef float TbV4 __attribute__((ext_vector_type(4)));
typedef TbV4 TbVec __attribute__((aligned(4)));   // rows may start at any float

// samples per fmaf chain: 16, 32, 64, 128, 256 from B = 64, 256, 1024, 4096, 16384
__host__ __device__ constexpr int tb_seg(int B)
{
    int s = 16;
    for (int b = 256; b <= B; b *= 4) s *= 2;
    return s;
}

struct TbArgs {
    long n, ldx, nblocks, ncols, ldp;
    int fill, carry;              // carried samples before / after the call
    int B, F, C;
    int ntiles;                   // workgroups of the power kernel that own columns
};

// Four samples of a row's stream from g in the call's coordinates: g >= 0 is x[g], g < 0 the carried samples
__device__ __forceinline__ TbV4 tb_load4(const float* __restrict__ xr, const float* __restrict__ hr, int fill, long g)
{
    if (g >= 0) return *reinterpret_cast<const TbVec*>(xr + g);
    TbV4 v;
#pragma unroll
    for (int u = 0; u < 4; u++) v[u] = g + u >= 0 ? xr[g + u] : hr[fill + g + u];
    return v;
}

template <int M, bool SPLIT>
__global__ void __launch_bounds__(kTbThreads)
    k_tonebank_power(const TbArgs a, const float* __restrict__ x, const float* __restrict__ hist,
                     float* __restrict__ hist_out, const TbV4* __restrict__ tab, float* __restrict__ power)
{
    __shared__ double part[SPLIT ? 3 * 16 * 64 : 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int B = a.B, fill = a.fill;
    if ((int)blockIdx.x >= a.ntiles) {                // a row's next carry: the last a.carry samples of its stream
        const int row = (int)blockIdx.x - a.ntiles;
        const float* __restrict__ xr = x + (long)row * a.ldx;
        const float* __restrict__ hr = hist + (long)row * B;
        float* __restrict__ ho = hist_out + (long)row * B;
        const long first = a.n - a.carry;             // in the call's coordinates; >= -fill
        for (int i = tid; i < a.carry; i += kTbThreads) {
            const long g = first + i;
            ho[i] = g >= 0 ? xr[g] : hr[fill + g];
        }
        return;
    }
    const long tile = SPLIT ? (long)blockIdx.x : (long)blockIdx.x * 4 + wave;
    if (tile * 32 >= a.ncols) return;                 // a whole wave (never with SPLIT: every tile has a column)
    const long col = tile * 32 + (lane & 31);
    const bool valid = col < a.ncols;
    const int h = lane >> 5;
    const long row = valid ? col / a.nblocks : 0, blk = valid ? col - row * a.nblocks : 0;
    const float* __restrict__ xr = x + row * a.ldx;
    const float* __restrict__ hr = hist + row * B;
    const long g0 = blk * B - fill + 4 * h;           // this lane's first sample; below 0 only in a row's first block
    const TbV4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};

    const int S = tb_seg(B), nseg = (B + S - 1) / S;
    int s_lo = 0, s_hi = nseg;
    if (SPLIT) {
        const int q = (nseg + 3) / 4;
        s_lo = min(wave * q, nseg);
        s_hi = min(s_lo + q, nseg);
    }
    double tot[M][16];
#pragma unroll
    for (int m = 0; m < M; m++)
#pragma unroll
        for (int r = 0; r < 16; r++) tot[m][r] = 0.0;

    // one pass over the wave's samples, eight at a time, the next eight's loads in flight; a
    // segment ends where the sample index reaches a multiple of S (a power of two) or the end
    const int i_lo = s_lo * S, i_hi = min(s_hi * S, B);
    TbAcc acc[M];
#pragma unroll
    for (int m = 0; m < M; m++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[m][r] = 0.0f;
    TbV4 xv = zero4, tv[M];
    if (i_lo < i_hi) {
        if (valid) xv = tb_load4(xr, hr, fill, g0 + i_lo);
#pragma unroll
        for (int m = 0; m < M; m++) tv[m] = tab[((long)(i_lo >> 3) * M + m) * 64 + lane];
    }
    for (int i = i_lo; i < i_hi; i += 8) {
        const int in = min(i + 8, i_hi - 8);          // the last step loads its own samples again
        TbV4 xn = zero4, tn[M];
        if (valid) xn = tb_load4(xr, hr, fill, g0 + in);
#pragma unroll
        for (int m = 0; m < M; m++) tn[m] = tab[((long)(in >> 3) * M + m) * 64 + lane];
#pragma unroll
        for (int u = 0; u < 4; u++)
#pragma unroll
            for (int m = 0; m < M; m++) acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(tv[m][u], xv[u], acc[m], 0, 0, 0);
        if (((i + 8) & (S - 1)) == 0 || i + 8 >= i_hi) {
#pragma unroll
            for (int m = 0; m < M; m++)
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    tot[m][r] = tot[m][r] + (double)acc[m][r];
                    acc[m][r] = 0.0f;
                }
        }
        xv = xn;
#pragma unroll
        for (int m = 0; m < M; m++) tv[m] = tn[m];
    }

    if (SPLIT) {                                      // wave 0 adds the four waves' sums in wave order, a row tile at a time
#pragma unroll
        for (int m = 0; m < M; m++) {
            if (wave > 0) {
#pragma unroll
                for (int r = 0; r < 16; r++) part[((wave - 1) * 16 + r) * 64 + lane] = tot[m][r];
            }
            __syncthreads();
            if (wave == 0) {
                for (int w = 0; w < 3; w++)
#pragma unroll
                    for (int r = 0; r < 16; r++) tot[m][r] = tot[m][r] + part[(w * 16 + r) * 64 + lane];
            }
            __syncthreads();
        }
        if (wave > 0) return;
    }
    if (!valid) return;
    float* __restrict__ pw = power + row * a.ldp + blk * a.F;
#pragma unroll
    for (int m = 0; m < M; m++)
#pragma unroll
        for (int hi = 0; hi < 2; hi++)
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const int k = 16 * m + 8 * hi + 4 * h + b;
                const float re = (float)tot[m][8 * hi + b], im = (float)tot[m][8 * hi + 4 + b];
                if (k < a.F) pw[k] = fmaf(re, re, im * im);
            }
}

__global__ void __launch_bounds__(kTbThreads)
    k_tonebank_detect(const TbArgs a, float floor, double dominance, int hold, const int8_t* __restrict__ want,
                      const int* __restrict__ since_in, int* __restrict__ since_out, const float* __restrict__ power,
                      int8_t* __restrict__ tone, long ldt, uint8_t* __restrict__ open, long ldo)
{
    __shared__ uint8_t flag[kTbThreads];
    const int t = threadIdx.x, row = blockIdx.y, F = a.F;
    const long tile0 = (long)blockIdx.x * kTbDetTile;
    const long b = tile0 - kTbHalo + t;
    const bool lastwg = blockIdx.x == gridDim.x - 1;
    bool acc = false;
    int best = -1;
    if (b >= 0 && b < a.nblocks && (t >= kTbHalo - hold || lastwg)) {
        const float* __restrict__ p = power + (long)row * a.ldp + b * F;
        int ks = 0;
        float pm = p[0];
        bool fin = isfinite(pm);
        for (int k = 1; k < F; k++) {
            const float v = p[k];
            fin = fin && isfinite(v);
            if (v > pm) {
                pm = v;
                ks = k;
            }
        }
        double others = 0.0;
        for (int k = 0; k < F; k++)
            if (k != ks) others = others + (double)p[k];
        const bool hit = fin && pm > floor && (double)pm * (double)(F - 1) > dominance * others;
        const int w = want[row];
        best = hit ? ks : -1;
        acc = hit && (w < 0 || w == ks);
    }
    flag[t] = acc ? 1 : 0;
    __syncthreads();
    const int since = since_in[row];
    if (t >= kTbHalo && b < a.nblocks) {
        bool op = false;
        for (int d = 0; d <= hold; d++) {
            if (b - d < 0) {                          // before the call: the last accepted block is -1 - since
                op = op || (long)since <= (long)hold - b - 1;
                break;
            }
            op = op || flag[t - d] != 0;
        }
        tone[(long)row * ldt + b] = (int8_t)best;
        open[(long)row * ldo + b] = op ? 1 : 0;
    }
    if (lastwg && t == 0) {                           // blocks since the last accepted one, saturating
        int next = kTonebankSat;
        for (int d = 0; d < kTonebankSat; d++) {
            const long bb = a.nblocks - 1 - d;
            if (bb < 0) {
                next = (int)min((long)since + a.nblocks, (long)kTonebankSat);
                break;
            }
            if (flag[bb - tile0 + kTbHalo]) {
                next = d;
                break;
            }
        }
        since_out[row] = next;
    }
}

__global__ void __launch_bounds__(kTbThreads)
    k_tonebank_gate(const TbArgs a, const float* __restrict__ x, const float* __restrict__ hist,
                    const uint8_t* __restrict__ open, long ldo, float* __restrict__ y, long ldy)
{
    const int row = blockIdx.y, fill = a.fill;
    const float* __restrict__ xr = x + (long)row * a.ldx;
    const float* __restrict__ hr = hist + (long)row * a.B;
    const uint8_t* __restrict__ orow = open + (long)row * ldo;
    float* __restrict__ yr = y + (long)row * ldy;
    const long total = a.nblocks * a.B, base = (long)blockIdx.x * kTbGateTile;
    const TbV4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 4
    for (int it = 0; it < kTbGateTile / (4 * kTbThreads); it++) {
        const long o = base + ((long)it * kTbThreads + threadIdx.x) * 4;   // B is a multiple of 64: four samples, one block
        if (o >= total) break;
        const bool op = orow[o / a.B] != 0;
        *reinterpret_cast<TbVec*>(yr + o) = op ? tb_load4(xr, hr, fill, o - fill) : zero4;
    }
}

// the matrix row of tone k's cosine (part 0) or sine (part 1): see the head of the file
inline int tb_row(int k, int part)
{
    const int m = k >> 4, t = k & 15;
    return 32 * m + 16 * (t >> 3) + 8 * part + 4 * ((t >> 2) & 1) + (t & 3);
}

template <int M>
void tb_power(const TbArgs& a, bool split, unsigned grid, hipStream_t s, const TonebankCall& c)
{
    if (split)
        hipLaunchKernelGGL((k_tonebank_power<M, true>), dim3(grid), dim3(kTbThreads), 0, s, a, c.x, c.hist, c.hist_out,
                           (const TbV4*)c.tab, c.power);
    else
        hipLaunchKernelGGL((k_tonebank_power<M, false>), dim3(grid), dim3(kTbThreads), 0, s, a, c.x, c.hist, c.hist_out,
                           (const TbV4*)c.tab, c.power);
}

} // namespace

int tonebank_tile(int B) { return B >= kTbSplitB ? 32 : 128; }

void tonebank_pack(int F, int B, const float* tc, const float* ts, std::vector<float>& out)
{
    const int M = (F + 15) / 16;
    std::vector<int> tone(32 * M, -1), part(32 * M, 0);
    for (int k = 0; k < F; k++)
        for (int p = 0; p < 2; p++) {
            tone[tb_row(k, p)] = k;
            part[tb_row(k, p)] = p;
        }
    out.assign((size_t)B * 32 * M, 0.0f);
    for (int q = 0; q < B / 8; q++)
        for (int m = 0; m < M; m++)
            for (int l = 0; l < 64; l++) {
                const int R = 32 * m + (l & 31), k = tone[R];
                if (k < 0) continue;
                const float* src = (part[R] ? ts : tc) + (size_t)k * B + 8 * q + 4 * (l >> 5);
                std::copy_n(src, 4, &out[(((size_t)q * M + m) * 64 + l) * 4]);
            }
}

void tonebank(const TonebankCall& c, hipStream_t s)
{
    if (c.n == 0) return;
    LDSP_REQUIRE(c.C >= 1 && c.C <= kTonebankMaxC, "tonebank: row count out of range");
    LDSP_REQUIRE(c.B >= kTonebankMinB && c.B <= kTonebankMaxB && c.B % 64 == 0, "tonebank: block length out of range");
    LDSP_REQUIRE(c.F >= kTonebankMinF && c.F <= kTonebankMaxF, "tonebank: tone count out of range");
    LDSP_REQUIRE(c.hold >= 0 && c.hold <= kTonebankMaxHold, "tonebank: hold out of range");
    LDSP_REQUIRE(c.n < ((size_t)1 << 36), "tonebank: call too long");
    LDSP_REQUIRE(c.ldx >= c.n && c.fill < (size_t)c.B, "tonebank: bad call geometry");
    LDSP_REQUIRE(c.nblocks == (c.fill + c.n) / c.B, "tonebank: block count does not match the call");
    LDSP_REQUIRE(c.ldp >= c.nblocks * c.F && c.ldt >= c.nblocks && c.ldo >= c.nblocks &&
                     (!c.y || c.ldy >= c.nblocks * c.B),
                 "tonebank: output row stride below the call's blocks");
    TbArgs a;
    a.n = (long)c.n;
    a.ldx = (long)c.ldx;
    a.nblocks = (long)c.nblocks;
    a.ncols = a.nblocks * c.C;
    a.ldp = (long)c.ldp;
    a.fill = (int)c.fill;
    a.carry = (int)((c.fill + c.n) % c.B);
    a.B = c.B;
    a.F = c.F;
    a.C = c.C;
    const int T = tonebank_tile(c.B);
    a.ntiles = (int)((a.ncols + T - 1) / T);
    {
        LDSP_PROF(s, "k_tonebank_power");
        const unsigned grid = (unsigned)(a.ntiles + c.C);
        const bool split = c.B >= kTbSplitB;
        switch ((c.F + 15) / 16) {
        case 1: tb_power<1>(a, split, grid, s, c); break;
        case 2: tb_power<2>(a, split, grid, s, c); break;
        case 3: tb_power<3>(a, split, grid, s, c); break;
        default: tb_power<4>(a, split, grid, s, c); break;
        }
        LDSP_HIP(hipGetLastError());
    }
    if (c.nblocks == 0) return;
    {
        LDSP_PROF(s, "k_tonebank_detect");
        const unsigned grid = (unsigned)((a.nblocks + kTbDetTile - 1) / kTbDetTile);
        hipLaunchKernelGGL(k_tonebank_detect, dim3(grid, (unsigned)c.C), dim3(kTbThreads), 0, s, a, c.floor, c.dominance,
                           c.hold, c.want, c.since, c.since_out, (const float*)c.power, c.tone, (long)c.ldt, c.open,
                           (long)c.ldo);
        LDSP_HIP(hipGetLastError());
    }
    if (c.y) {
        LDSP_PROF(s, "k_tonebank_gate");
        const unsigned grid = (unsigned)((a.nblocks * a.B + kTbGateTile - 1) / kTbGateTile);
        hipLaunchKernelGGL(k_tonebank_gate, dim3(grid, (unsigned)c.C), dim3(kTbThreads), 0, s, a, c.x, c.hist,
                           (const uint8_t*)c.open, (long)c.ldo, c.y, (long)c.ldy);
        LDSP_HIP(hipGetLastError());
    }
}

} // namespace k
} // namespace ldsp
