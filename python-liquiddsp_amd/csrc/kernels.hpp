// kernels.hpp -- host launchers for the gfx950 kernels of libldsp.
// All pointers are device pointers; every launcher only enqueues on `s`.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace ldsp {
namespace k {

// ------------------------------------------------------------------ FIR
// y[i] = scale * sum_{k<L} h[k] xv[i-k], xv[j<0] = hist[j + L - 1]; writes the
// new history (last L-1 samples of xv) to hist_out.  taps_pad has
// ceil(L/16)*16 floats (zero padded).  fast: register-blocked FMA kernel;
// exact: liquid dotprod order (oldest sample first, separate mul and add).
constexpr int kFirMaxTaps = 8192;
void fir_fast(bool cplx, const void* x, const void* hist, void* hist_out, size_t n,
              const float* taps_pad, int L, float scale, void* y, hipStream_t s);
void fir_exact(bool cplx, const void* x, const void* hist, void* hist_out, size_t n,
               const float* taps_rev, int L, float scale, void* y, hipStream_t s);
// history update only (n == 0 calls skip the kernels)

// Overlap-save FFT convolution (complex samples, real taps), k_firfft.hip.
// P = history samples per window (L - 1 <= P <= 512, multiple of 64); the
// window has fir_fft_points(P) = 512 (P <= 128) or 1024 points.
// H[N] = scale * FFT(h) / N for that N; tw = Stockham twiddles
// exp(-2 pi i r k / (Ns R)) laid out [pass][r-1][k]:
//   N = 512 : (Ns, R) = (8, 8), (64, 8)      -> kFft512Tw entries
//   N = 1024: (Ns, R) = (16, 16), (256, 4)   -> kFft1024Tw entries
constexpr int kFft512Tw = 7 * 8 + 7 * 64;
constexpr int kFft1024Tw = 15 * 16 + 3 * 256;
int fir_fft_points(int P);
// Optional NCO mix fused into the window loads (table NCO, nco_crcf_mix_block_*):
// sample i enters as x[i] e^{-+j theta}, theta = theta0 + i dtheta; hist then
// holds mixed samples, like the filter's own history after a separate mix.
struct NcoFuse {
    uint32_t theta0, dtheta;
    bool down;
    const float* table;   // device sine table (1024)
};
void fir_fft(const void* x, const void* hist, void* hist_out, size_t n, int L, int P, const void* H, const void* tw,
             void* y, hipStream_t s, const NcoFuse* nco = nullptr);

// ------------------------------------------------------------------ resampler
struct ResampPlan {
    uint64_t P0;          // phase at call start (resamp "phase", < 2^24 + step)
    uint32_t step;        // round(2^24 / rate)
    int bits_index;       // 24 - log2(npfb)
    int sub_len;          // taps per branch (2m)
    int npfb;
    size_t K;             // outputs of this call
    int KB;               // outputs per workgroup
    int span_max;         // LDS samples per workgroup
    int tile = 0;         // 1: k_resamp_tile (span streamed into LDS with 16-byte loads), KB from resamp_tile_outputs
};
// Outputs per workgroup of the tile kernel (0: its LDS would not fit; use the others).
int resamp_tile_outputs(uint32_t step, int sub_len, int npfb, bool cplx, bool real_taps);
// The kernel of a call, decided on the host from the plan alone: the tile kernel
// when its LDS fits; else k_resamp_direct (one output per thread, kResampDirectOutputs
// per workgroup) while the branch table fits 64 KiB of LDS; else k_resamp, which stages
// each workgroup's span and also serves the calls without outputs (history only).
enum ResampKernel { kResampTile = 0, kResampDirect = 1, kResampStaged = 2 };
constexpr int kResampDirectOutputs = 256;
// Fills KB, span_max and tile from step, sub_len and npfb (host logic only).
void resamp_plan(ResampPlan& p, bool cplx, bool real_taps);
ResampKernel resamp_kernel(const ResampPlan& p, bool cplx, bool real_taps);
// sub: [npfb][sub_len] branch taps reversed (cccf: complex64 with imag 0; rrrf, crcf: float)
void resamp(bool cplx, bool real_taps, const void* x, const void* hist, void* hist_out, size_t n, const float* sub,
            const ResampPlan& p, void* y, hipStream_t s);

// ------------------------------------------------------------------ NCO
void nco_mix(const void* x, void* y, size_t n, uint32_t theta0, uint32_t dtheta, const float* table,
             bool down, int type, hipStream_t s);

// ------------------------------------------------------------------ IIR
// Structure of one IIR filter for the kernels.  SOS: nsos sections b[3],a[3]
// (a0 == 1); TF: nb, na coefficients (a0 == 1), nv = max(nb, na).
constexpr int kIirMaxState = 16;
struct IirDesc {
    int sos;              // 1 SOS cascade, 0 TF
    int nsos;
    int nb, na, nv;
    int D;                // state dimension (SOS: 2 nsos, TF: nv - 1)
    const float* b;       // device coefficients
    const float* a;
};
// Sequential float32 evaluation (bit-exact with the liquid recursion).
// state: float[2][3*nsos] (SOS) or float[2][nv] (TF); cplx -> 2 components.
void iir_seq(bool cplx, const IirDesc& d, const void* x, size_t n, float* state, void* y, hipStream_t s);
// Sections per cascade of the exact kernel below.
constexpr int kIirSectMaxSos = 8;
// The same recursion with one wave per section and one workgroup per (object,
// component) (k_iir_sect.hip); mergeable in many-calls.  iir_seq uses it for SOS
// cascades of <= kIirSectMaxSos sections.
void iir_sect(bool cplx, const IirDesc& d, const void* x, size_t n, float* state, void* y, hipStream_t s);
int iir_sect_tile(int nsos);           // its tile: 1024 samples while the rings fit the CU's LDS, else 512
// What iir_seq launches for d (host logic only): k_iir_sect with tiles of
// sect_tile samples, or -- sect_tile == 0 -- k_iir_seq<size_class>.  size_class
// (2, 4 or 17 sections / coefficients) also selects the iir_spec kernels.
struct IirSeqKernel {
    int sect_tile, size_class;
};
IirSeqKernel iir_seq_kernel(const IirDesc& d);
int iir_sect_trace(void* dev_buf);     // diagnostics: ldsp_debug_iir_sect_trace
// Float64 chunked linear scan.  state64: double[2][D] (the DF-II delay line in
// the layout used by the scan); Apow: double[D*D] matrices: [0] = A^C,
// [1 + l] = A^{C G 2^l} prepared by the host (see IirScanPlan).
struct IirScanPlan {
    int C;                // samples per chunk
    long nchunks;
    int G;                // chunks per scan thread (1024 scan threads)
    int levels;           // 10 = log2(1024)
    const double* AC;     // A^C           [D*D]
    const double* AG;     // A^{C*G*2^l}    [levels][D*D]
    double* local;        // [nchunks][ncomp][D] scratch: chunk end state from zero
    double* carry;        // [nchunks][ncomp][D] scratch: chunk start state
};
void iir_scan(bool cplx, const IirDesc& d, const void* x, size_t n, double* state64, const IirScanPlan& p,
              void* y, hipStream_t s);
// Blocked float64 scan for state dimension D <= kIirBlkMaxD (k_iir_blk):
// chunks of 256 samples, 256 chunks per block.  hb/ha: host copies of the
// float32 coefficients (SOS [nsos][3] or TF [nb] / [na]), passed by value.
constexpr int kIirBlkMaxD = 8;
constexpr int kIirBlkChunk = 256;
constexpr int kIirBlkChunks = 256;
struct IirBlkPlan {
    long nchunks, nblk;
    int G;                // blocks per carry thread
    const double* AL;     // A^{256 * 2^l}, l = 0..7             [8][D*D]
    const double* AB;     // A^{65536}                            [D*D]
    const double* AG;     // A^{65536 * G * 2^l}, l = 0..9         [10][D*D]
    double* local;        // [nchunks][ncomp][D]
    double* blocal;       // [nblk][ncomp][D]
    double* bstart;       // [nblk][ncomp][D]
};
// iq16: x holds int16 (I, Q) pairs, converted on load as bytes_to_iq does
void iir_blk(bool cplx, const IirDesc& d, const float* hb, const float* ha, const void* x, size_t n, double* state64,
             const IirBlkPlan& p, void* y, hipStream_t s, bool iq16 = false);
// Single-pass float64 scan in modal coordinates (k_iir_modal.hip): the filter
// as M <= 8 parallel sections (one per pole pair or real pole) in direct form,
// w_n = u_n - a1 w_{n-1} - a2 w_{n-2}, y = d u + sum_k c1 w_{n-1} + c2 w_{n-2}
// (modal.hpp).  One wave = 64 chunks of kIirModalChunk samples; each unit's
// start state is the look-back sum over the J <= kIirModalJmax units before it
// (valid when max|lambda|^(2048 J) < 2^-70).  State layout (st_in / st_out,
// distinct buffers): double [ncomp][M][w_n, w_{n-1}].
constexpr int kIirModalMax = 8;
constexpr int kIirModalChunk = 32;
constexpr int kIirModalJmax = 64;
struct IirModalCoef {     // kernel argument
    int M;
    double a1[kIirModalMax], a2[kIirModalMax];   // section denominators
    double c1[kIirModalMax], c2[kIirModalMax];   // section outputs
    double d;                                    // direct term
};
struct IirModalPlan {
    int J;                // look-back depth (units)
    const double* PS;     // [6][M][4]   A_k^(32 * 2^l), l = 0..5 (2 x 2, row-major)
    const double* PL;     // [64][M][4]  A_k^(32 t), t = lane
    const double* PB;     // [J][M][4]   A_k^(2048 i)
    uint64_t* agg;        // [nunits][ncomp][M * 4] {32-bit half, epoch} granules (zeroed when allocated)
    uint32_t epoch;       // per call, never 0
    int recompute = 0;    // test hook: every wave recomputes its predecessors instead of reading them
    int one_xcd = 0;      // small call: every unit on the XCD of block 0 (a grid of 8 x units, the
                          // blocks of the other XCDs return at once), so no unit recomputes a predecessor
    int variant = 0;      // tuning builds only (timing experiments, wrong outputs): bit 0 no look-back,
                          // bit 1 no pass 2, bit 2 no pass 1 / scan; bit 3 stagger the first
                          // round of workgroups by (variant >> 4) sleeps (outputs unchanged)
};
// IIR -> resampler fusion (liquiddsp.filter_resample, k_iir_modal<RS>): each unit's
// filter outputs stay in LDS and feed the resampler outputs whose sub_len-sample
// window lies inside the unit (the resampler's own arithmetic, resamp_dev.hpp);
// the unit's first and last H = sub_len - 1 outputs go to `side`, from which
// k_iir_resamp_edges computes the outputs whose window straddles a unit boundary
// (and the resampler's new history).  The filter outputs never reach HBM.
struct IirResampFuse {
    const float* sub;     // [npfb][sub_len] branch taps, reversed (ResampObj::sub; complex interleaved if ctaps)
    uint64_t P0;          // the resampler's phase at the call's start
    uint32_t step;
    int bits_index, sub_len;
    int ctaps;            // complex taps (resamp_cccf, the ComplexResampler): rs_mac over both components
    long K;               // outputs of the call
    float* side;          // [units][2][H][ncomp]: head (first H) and tail (last H, right-aligned) outputs
    float* y;             // resampler outputs ([K][ncomp] floats)
};
size_t iir_resamp_side_bytes(size_t n, int sub_len, bool cplx);
void iir_modal_resamp(bool cplx, const IirModalCoef& cf, const void* x, size_t n, const double* st_in,
                      double* st_out, const IirModalPlan& p, const IirResampFuse& f, const void* hist,
                      void* hist_out, hipStream_t s);
long iir_modal_units(size_t n);   // workgroups (2048-sample look-back units) of a call
unsigned iir_modal_grid(size_t n, int one_xcd);   // workgroups launched: 8 x units in the one-XCD mode (7 of 8 return at once)
void iir_modal(bool cplx, const IirModalCoef& cf, const void* x, size_t n, const double* st_in, double* st_out,
               const IirModalPlan& p, void* y, hipStream_t s, bool iq16 = false);
// Speculative exact evaluation for fast-decaying filters: chunks start from a
// zero state W samples early; a verifier re-runs any chunk whose guessed
// start state differs bit-wise from its predecessor's end state.
struct SpecPlan {
    int C;                // samples per chunk
    int W;                // warm-up samples (exact)
    int Wa = 0;           // AGC: approximate warm-up before the exact one
    int rounds = 0;       // AGC: parallel repair rounds before the sequential verifier
    unsigned* dbg = nullptr;   // AGC debug: per-round re-run counters (LDSP_DEBUG_AGC)
    long nchunks;
    void* scratch;        // device scratch (states: start-guess and end per chunk)
    const void* hist = nullptr;   // AGC: the H input samples before x[0] (H > 0: every chunk speculative)
    int H = 0;
    int tsa = 0;          // AGC small call: every chunk approximates from the true state up to its start
                          // (2: one wave, which also checks and repairs the chunks in order;
                          // | 4: test hook, every chunk's start state 1 ulp off;
                          // | 8: test hook, chunk-parallel call: odd chunks start 1 ulp off)
};
// scratch for iir_spec: chunk states + verifier flag words
size_t spec_flags_offset(long nchunks, int ncomp, int fs);
size_t spec_scratch_bytes(long nchunks, int ncomp, int fs);
// true: k_iir_spec_chunks stages a workgroup's input window in LDS (it fits 64 KiB)
bool iir_spec_staged(bool cplx, const SpecPlan& p);
void iir_spec(bool cplx, const IirDesc& d, const void* x, size_t n, float* state, const SpecPlan& p, void* y,
              hipStream_t s);

// ------------------------------------------------------------------ AGC
struct AgcState {         // device-resident agc_crcf state
    float g, y2p, alpha, scale;
    int locked, mode;
    unsigned int timer, timeout;
    float threshold;
    int pad[3];           // test counters: [0] small-call in-kernel re-runs, [1] verifier re-runs, [2] runfix re-runs
};
constexpr int kAgcPow = 256;     // samples whose mean power sets a chunk's guessed gain
void agc_seq(const void* x, size_t n, AgcState* st, void* y, uint8_t* status, hipStream_t s);
size_t agc_scratch_bytes(long nchunks, int C);
// Chunk-parallel exact AGC in two halves.  Front: the chunks (reads only the
// parameters when p.H > 0, so it may run while the previous call's back half
// still advances the state).  Back: flag / repair rounds and the verifier
// against the true state, which it then advances.
void agc_spec_front(const void* x, size_t n, AgcState* st, const SpecPlan& p, void* y, uint8_t* status,
                    hipStream_t s);
void agc_spec_back(const void* x, size_t n, AgcState* st, const SpecPlan& p, void* y, uint8_t* status,
                   hipStream_t s);
// A speculative call's back half in two parts: the repair rounds over chunks
// 1.. (chunk 0 presumed right: they read only the chunk records, so they may
// run while the previous call is still producing the true state), then -- after
// it -- the verifier, which checks chunk 0 against the true state, re-runs
// whatever the rounds left and advances the state: the only AGC work on the
// chain from one call to the next.
void agc_spec_repair(const void* x, size_t n, AgcState* st, const SpecPlan& p, void* y, uint8_t* status,
                     hipStream_t s);
void agc_spec_verify(const void* x, size_t n, AgcState* st, const SpecPlan& p, void* y, uint8_t* status,
                     hipStream_t s);
// hist_out = the last m samples of (hist, x[0, n)) (complex), for the next call.
void delay_hist(const void* x, const void* hist, void* hist_out, size_t n, int m, hipStream_t s);

// ------------------------------------------------------------------ AmpModem
struct AmpState {         // device-resident PLL state
    uint32_t theta, dtheta;   // true loop state (written by the walker / sequential loop)
    float alpha, beta;
    uint32_t gth[2], gd[2];   // ping-pong guess of the state at the next call's start (candidate end state)
    uint32_t sq_batches;      // k_pll_seqc diagnostics, cumulative: candidate batches stepped,
    uint32_t sq_redone;       //   and batches with a step evaluated by pll_eval (an index left its window)
    // hand-off: every launch that writes theta / dtheta advances wepoch after them
    // (release); a walker launched early waits until wepoch equals its call's index
    uint32_t wepoch;
    uint32_t werr;            // 1: a walker's hand-off wait timed out (the host raises)
    unsigned long long wact;  // walker ticks (10 ns) from hand-off to end, cumulative
    unsigned long long wact_n;
    unsigned long long wait_ticks;   // bound of the hand-off wait (10 ns ticks; 1 s unless a test shortens it)
    uint32_t* herr;           // host-mapped flag the walker also sets on a timeout: checked at every call's
                              // entry, so a timed-out walk is never returned silently (capi.cpp amp_check_err)
};
// One AmpModem / BroadcastAM PLL call.  x0 = lowpass(x) (precomputed), x1 =
// delay_m(x) via hist (m samples before x[0]); writes Re(v1)/mod (carrier) or
// the final output (Costas) to y.  scratch (pll_scratch_bytes(n)) holds the
// candidate records of the chunk-parallel exact path (k_pll.hip).
struct PllCall {
    const void* x0;
    const void* x;
    const void* hist;     // m samples before x[0]
    void* hist_out;       // m samples before the next call's x[0]
    int m;
    size_t n;
    AmpState* st;
    int gcur;             // candidates start from st->gth/gd[gcur], leave the next guess in [1 - gcur]
    const float* table;
    float mod_index;
    int costas;
    int out_idx;          // 1: write each sample's table index (uint32 bits) instead of its output (SSB: the
                          //    Hilbert stage recomputes v1 from it)
    float alpha_host;
    float* y;
    void* scratch;
    uint32_t wexp;        // launches that wrote the PLL state before this call's (AmpState::wepoch)
};
size_t pll_scratch_bytes(size_t n);
size_t pll_stats_offset(size_t n);     // 4 x u64 walker counters inside the scratch (debug)
// True when the call runs as candidates + walker (else one sequential loop in pll_back).
bool pll_parallel(size_t n, int costas);
// Front half: the delay-line history for the next call and (parallel calls)
// the candidate chunks.  Reads only the guess state, never the true state, so
// it may run while the previous call's pll_back is still walking.
void pll_front(const PllCall& c, hipStream_t s);
int pll_margin_override(int log2_b);       // diagnostics: 0 = default; returns the previous value
// Back half: the exact walk over the candidates (or the sequential loop);
// reads and advances the true state, so it must follow the previous call's back half.
void pll_back(const PllCall& c, hipStream_t s);

// The interval fields of one walker entry record (k_pll_entries; host-callable so the
// CPU suite runs the kernel's own code: ldsp_debug_walk_fold).  u: the candidate's
// position in its table cell (22 bits), so the offset f of the true phase from the
// candidate's stays in the cell while f in [-u, 2^22 - 1 - u]; B: the margin; lne / rne:
// the gap to the previous / next entry is non-empty (|f| <= B needed across it); dk2:
// what a repair at this entry adds to f.
//   [lo, lo + W]: no event (the cell, cut to [-B, B] if lne or rne); the walker's
//       x = f - lo, event iff x >u W.
//   [fl, fh]: the pre-repair offsets at which a repair here is right -- the one
//       crossing possible while |f| < 2^21 (up if u >= 2^21, else down), cut to [-B, B]
//       if lne and to [-B - dk2, B - dk2] (f_post within B) if rne.
//   A repaired lane keeps its pre-repair x, so the walker's test over every lane is
//   x <=u W (not repaired) or x - amin <=u awidth (repaired, and rightly).  [fl, fh]
//   mostly starts where the cell ends (up: fl = hi + 1; down: fh = lo - 1), but not
//   always -- with only rne, the cell's side towards the crossing cut to +-B and dk2
//   pointing back inside it lies detached beyond a gap that must fail -- so the two
//   intervals are not folded into one.  An empty [fl, fh] is stored as amin = awidth
//   = 0: x = 0 is never a repaired lane's, so every repair at the entry fails.
struct WalkFold {
    int32_t lo;
    uint32_t W, amin, awidth;
};
__host__ __device__ inline WalkFold pll_walk_fold(uint32_t u, int32_t B, bool lne, bool rne, uint32_t dk2)
{
    long lo = -(long)u, hi = (1l << 22) - 1 - (long)u;
    if (lne || rne) {
        lo = lo > -(long)B ? lo : -(long)B;
        hi = hi < (long)B ? hi : (long)B;
    }
    const bool up = u >= (1u << 21);
    long fl = up ? (1l << 22) - (long)u : -(1l << 22) - (long)u;
    long fh = fl + (1l << 22) - 1;
    if (lne) {
        fl = fl > -(long)B ? fl : -(long)B;
        fh = fh < (long)B ? fh : (long)B;
    }
    if (rne) {
        const long d2 = (long)(int32_t)dk2;
        fl = fl > -(long)B - d2 ? fl : -(long)B - d2;
        fh = fh < (long)B - d2 ? fh : (long)B - d2;
    }
    const bool any = fl <= fh;
    WalkFold r;
    r.lo = (int32_t)lo;
    r.W = (uint32_t)(hi - lo);
    r.amin = any ? (uint32_t)(fl - lo) : 0u;
    r.awidth = any ? (uint32_t)(fh - fl) : 0u;
    return r;
}

// ------------------------------------------------------------------ debug
void math_eval(int fn, const float* a, const float* b, float* y, size_t n, hipStream_t s);

// k_misc.hip: bytes_to_iq, delay line, frequency discriminator
void bytes_to_iq(const void* x, void* y, size_t n, hipStream_t s);
void delay(bool cplx, const void* x, const void* hist, void* hist_out, size_t n, int D, void* y, hipStream_t s);
void freqdem(const void* x, const void* prev, void* prev_out, size_t n, float ref, float* y, hipStream_t s);
// AmpModem usb / lsb: v1 = delay_m(x) mixed down by the per-sample table index idx
// (the PLL stage's out_idx output); Hilbert c2r over x (4M - 1 samples of history
// before x[0]) -> 0.5 * sideband / mod_index.
void ssb_v1(const void* idx, const void* x, const void* dhist, int m, const float* table, size_t n, void* v1,
            hipStream_t s);
void ssb_c2r(const void* x, const void* hist, size_t n, const float* hq, int M, int usb, float mod_index, float* y,
             hipStream_t s);
// k_hilbert.hip: firhilbf for SSBDemod / HilbertTransform.  op as LDSP_HILB_*;
// x: n input samples (C2R, INTERP complex64; R2C, DECIM float32, n even for
// DECIM); hist / hist_out: the H input samples before x[0] / before the next
// call's x[0], in the input's layout (H = 4M - 1; INTERP 2M - 1), distinct
// buffers; hq: the 2M quadrature taps followed by kHilbTapPad readable floats
// (the kernel fetches taps one step ahead).  C2R writes the lower sideband to y0
// and the upper to y1 (either may be null); the other ops write y0.
enum HilbOp { kHilbR2C = 0, kHilbC2R = 1, kHilbDecim = 2, kHilbInterp = 3 };
constexpr int kHilbTapPad = 4;
constexpr int kHilbMaxM = 64;         // semi-length bound (the LDS planes), as AmpModem's Hilbert stage
constexpr int kHilbTile = 2048;       // input samples per workgroup (INTERP: half as many)
void hilbert(int op, const void* x, const void* hist, void* hist_out, size_t n, const float* hq, int M, void* y0,
             void* y1, hipStream_t s);
// k_chan.hip: polyphase analysis filter bank (Channelizer).  M channels (a
// power of two, 4 .. 256), decimation D = M or M / 2, P = ceil(L / M) <= kChanMaxP
// taps per branch.  x: n complex64 samples; hist / hist_out: the P M - 1 samples
// before x[0] / before the next call's x[0], distinct buffers; taps: the
// prototype zero-padded to kChanMaxP * M floats; tw[j] = exp(2 pi i j / M), j < M.
// The call's frames are at x[skip + c D], c < ncols = ceil((n - skip) / D) (0 when
// n <= skip); parity: that of the first frame's absolute index (the D = M / 2
// sign).  y[k * ld + c] receives channel k.  n = 0 launches nothing.
// iq16 (here, in DdcCall and in SpgramCall): x holds n int16 (I, Q) pairs,
// 4-byte aligned, converted on load as bytes_to_iq does; hist / hist_out are
// complex64 either way.
constexpr int kChanMaxP = 17;
constexpr int chan_frames(int M) { return M >= 256 ? 32 : 4096 / M; }   // output frames per workgroup
struct ChanCall {
    const void* x;
    const void* hist;
    void* hist_out;
    size_t n, skip, ncols, ld;
    int parity, P;
    const float* taps;
    const void* tw;
    float scale;
    void* y;
    bool iq16 = false;
};
void chan(int M, int D, const ChanCall& c, hipStream_t s);
// k_ddc.hip: tuned decimating filter bank (Downconverter).  C <= kDdcMaxC tuners,
// decimation 2 <= D <= kDdcMaxD, one real prototype of L <= kChanMaxP D taps.
// x: n complex64 samples; hist / hist_out: the L - 1 raw samples before x[0] /
// before the next call's x[0], distinct buffers (at least one readable sample
// when L = 1).  The call's columns are at x[skip + c D], c < ncols as k_chan's;
// col0: the absolute index of the first (the rotation's phase).  With
// TB = ddc_block(C) tuners per block, taps holds the complex taps
// g_c[j] = h[j] exp(+2 pi i ((j w_c) mod 2^32) / 2^32) as
// [ceil(C / TB)][L][TB] (re, im) pairs indexed by k = L - 1 - j, zero for the
// tuners past C, words the C frequency words (padded likewise) and slots the L
// LDS slots ddc_slot(D, L, k).  y[c * ld + col] receives tuner c.  n = 0
// launches nothing.
constexpr int kDdcMaxC = 64;
constexpr int kDdcMaxD = 256;
constexpr int ddc_block(int C) { return C >= 3 ? 4 : C; }   // tuners a wave carries at once
int ddc_frames(int D, int L);                               // output columns per workgroup
int ddc_slot(int D, int L, int k);                          // where the staged span keeps offset k of column 0
struct DdcCall {
    const void* x;
    const void* hist;
    void* hist_out;
    size_t n, skip, ncols, ld;
    uint64_t col0;
    int C, L;
    const void* taps;
    const int* slots;
    const uint32_t* words;
    float scale;
    void* y;
    bool iq16 = false;
};
void ddc(int D, const DdcCall& c, hipStream_t s);
// k_fmbank.hip: FM discriminator and decimating real FIR over bank rows (FMBank).
// C <= kFmbankMaxC rows, decimation 1 <= D <= kFmbankMaxD, a real prototype of
// L <= kChanMaxP D taps; L = 0 (D = 1 only) is the discriminator alone.
// x: row c is n complex64 samples at x + c * ldx.  dhist / dhist_out: per row the
// L - 1 discriminator values before the call's first / before the next call's
// first, [C][L - 1]; prev / prev_out: per row the raw sample before x[c][0] /
// the call's last; distinct buffers.  The call's columns are at sample
// skip + m D, m < ncols, as k_chan's.  taps: the host's table [D][ceil(L / D)],
// t[r][q] = h[L - 1 - (q D + r)] (zero where q D + r >= L).  y[c * ldy + m]
// receives row c.  n = 0 launches nothing.
constexpr int kFmbankMaxC = 256;
constexpr int kFmbankMaxD = 64;
int fmbank_frames(int D, int L);                            // output columns per workgroup
struct FmbankCall {
    const void* x;
    const float* dhist;
    float* dhist_out;
    const void* prev;
    void* prev_out;
    size_t n, ldx, skip, ncols, ldy;
    int C, L;
    const float* taps;
    float ref, scale;
    float* y;
};
void fmbank(int D, const FmbankCall& c, hipStream_t s);
// k_audiobank.hip: de-emphasis and polyphase resampler over bank rows (AudioBank).
// C <= kAudiobankMaxC rows of float32, row c's n samples at x + c * ldx; the
// resampler's schedule (P0, step, bits_index) and branches (sub_len = 2m <=
// 2 kAudiobankMaxM taps each, npfb sub_len <= kAudiobankMaxTaps) are
// ResampPlan's.  sub: the branch taps reversed as the resampler kernels take
// them, rows padded to sub_len + 1 floats, [npfb][sub_len + 1].  J > 0: de-emphasis
// e = b0 sum a^j u with a warm-up of J <= kAudiobankMaxJ samples (a^J <= 2^-30, J
// from audiobank_warmup: whole blocks of the kernel's de-emphasis grid); J = 0: none.  seen: the samples per row before the call (the de-emphasis grid is
// absolute).  hist / hist_out: per row the H = audiobank_hist(sub_len, J) raw
// samples before x[c][0] / before the next call's first, [C][H], distinct buffers.
// y[c * ldy + k], k < K, receives row c: float32, or int16 with pcm16 (ldy in
// samples of the output type).  n = 0 launches nothing.
constexpr int kAudiobankMaxC = 256;
constexpr int kAudiobankMaxM = 32;
constexpr int kAudiobankMaxTaps = 8192;
constexpr int kAudiobankMaxJ = 693;                         // a^J <= 2^-30 at tau sample_rate = 32 takes 666
int audiobank_warmup(int J);                                // J rounded up to whole blocks
int audiobank_hist(int sub_len, int J);
int audiobank_tile(uint32_t step, int sub_len, int npfb, int J);   // outputs per workgroup
struct AudiobankCall {
    const float* x;
    const float* hist;
    float* hist_out;
    size_t n, ldx, K, ldy;
    uint64_t P0, seen;
    uint32_t step;
    int bits_index, sub_len, npfb;
    int C, J, H;
    double a, b0;
    const float* sub;
    float scale;
    int pcm16;
    void* y;
};
void audiobank(const AudiobankCall& c, hipStream_t s);
// k_sqbank.hip: per-row level and squelch gate over bank rows (SquelchBank).
// C <= kSqbankMaxC rows of complex64, row c's n samples at x + c * ldx; blocks of
// kSqbankMinB <= B <= kSqbankMaxB samples.  The call's stream per row is the
// fill < B carried samples (hist, [C][B]) followed by x; it holds nblocks =
// (fill + n) / B whole blocks, and hist_out (a distinct buffer) receives the
// (fill + n) mod B samples after them.  p: scratch for nblocks doubles per row.
// st: per row the smoothed power, the mode and the timer, updated in place;
// thr: per row the linear threshold.  level[c * ldl + b] and status[c * lds + b],
// b < nblocks, receive row c; y (may be NULL: the gate is not launched) receives
// nblocks B samples per row at y + c * ldy.  n = 0 launches nothing.
constexpr int kSqbankMaxC = 256;
constexpr int kSqbankMinB = 16;
constexpr int kSqbankMaxB = 4096;
int sqbank_tile(int B);                                     // blocks per workgroup of k_sqbank_power
struct SqState {
    double s;
    int mode, timer;
};
struct SqbankCall {
    const void* x;
    const void* hist;
    void* hist_out;
    size_t n, ldx, fill, nblocks, lds, ldl, ldy;
    int C, B, timeout;
    double alpha;
    const float* thr;
    SqState* st;
    double* p;
    uint8_t* status;
    float* level;
    void* y;
};
void sqbank(const SqbankCall& c, hipStream_t s);
// k_agcbank.hip: look-ahead hang AGC over bank rows (AGCBank).  C <= kAgcbankMaxC
// rows of float32 or (cplx) complex64, row c's n samples at x + c * ldx; blocks of
// kAgcbankMinB <= B <= kAgcbankMaxB samples.  The call's stream per row is the
// fill < 2B carried samples (hist, [C][2B]) followed by x: the samples not yet
// emitted, whose first B are the block tracked last when pend = 1.  The call
// tracks the nt = (fill + n - pend B) / B blocks after that one and emits the
// ne = max(pend + nt - 1, 0) blocks from the stream's start; hist_out (a distinct
// buffer) receives the fill + n - ne B samples after them.  peak_q[c * ldq + b]
// and gain_q[c * ldq + b], b < nt, receive row c; gains ([C][ldg], ldg >=
// pend + nt + 1) is scratch for the boundary gain before the call and the
// blocks' g; y receives ne B samples per row at y + c * ldy.  Per row, updated in
// place: level (the tracker), tail ([C][256], the last H peaks, newest last) and
// edge ([C][2]: the boundary gain before the pending block, the pending block's
// g).  target: per row, units; Gmax and d: units (agc_track.hpp).  n = 0 launches
// nothing.
constexpr int kAgcbankMaxC = 256;
constexpr int kAgcbankMinB = 16;
constexpr int kAgcbankMaxB = 4096;
constexpr int kAgcbankTail = 256;
int agcbank_tile(int B, int cplx);                          // blocks per workgroup of k_agcbank_peak / _apply
struct AgcbankCall {
    const void* x;
    const void* hist;
    void* hist_out;
    size_t n, ldx, fill, nt, ne, ldq, ldg, ldy;
    int C, B, H, pend, cplx;
    int32_t Gmax;
    int64_t d;
    const int32_t* target;
    int32_t* level;
    int32_t* tail;
    float* edge;
    int32_t* peak_q;
    int32_t* gain_q;
    float* gains;
    void* y;
};
void agcbank(const AgcbankCall& c, hipStream_t s);
// k_tonebank.hip: per-row tone detector and tone squelch over bank rows
// (ToneBank).  C <= kTonebankMaxC rows of float32, row c's n samples at
// x + c * ldx; blocks of B samples (a multiple of 64), F tones.  The call's
// stream per row is the fill < B carried samples (hist, [C][B]) followed by x, as
// k_sqbank.hip's; hist_out (a distinct buffer) receives the (fill + n) mod B
// samples after the nblocks whole blocks.  tab: the tables in the power kernel's
// layout (tonebank_pack, from tc and ts, [F][B] each).  power[c * ldp + b F + k],
// tone[c * ldt + b] and open[c * ldo + b], b < nblocks, receive row c (none may
// be NULL); y (may be NULL: the gate is not launched) receives nblocks B samples
// per row at y + c * ldy.  want: per row;  since / since_out (distinct buffers):
// per row the blocks since the last accepted one, at most kTonebankSat.  n = 0
// launches nothing.
constexpr int kTonebankMaxC = 256;
constexpr int kTonebankMinB = 64;
constexpr int kTonebankMaxB = 16384;
constexpr int kTonebankMinF = 2;
constexpr int kTonebankMaxF = 64;
constexpr int kTonebankMaxHold = 64;
constexpr int kTonebankSat = kTonebankMaxHold + 1;
int tonebank_tile(int B);                                   // columns (row, block pairs) per workgroup of k_tonebank_power
void tonebank_pack(int F, int B, const float* tc, const float* ts, std::vector<float>& out);
struct TonebankCall {
    const float* x;
    const float* hist;
    float* hist_out;
    const float* tab;
    size_t n, ldx, fill, nblocks, ldp, ldt, ldo, ldy;
    int C, B, F, hold;
    float floor;
    double dominance;
    const int8_t* want;
    const int* since;
    int* since_out;
    float* power;
    int8_t* tone;
    uint8_t* open;
    float* y;
};
void tonebank(const TonebankCall& c, hipStream_t s);
// k_stbank.hip: FM stereo decoder over bank rows (StereoBank).  C <= kStbankMaxC
// rows of float32 multiplex, row c's n samples at x + c * ldx; decimation
// 1 <= D <= kStbankMaxD, two real prototypes of L <= kStbankMaxL taps.  hist /
// hist_out: per row the L - 1 raw samples before x[c][0] / before the next
// call's first, [C][L - 1], distinct buffers (at least one readable sample when
// L = 1).  The call's columns are at sample skip + m D, m < ncols, as k_chan's.
// taps: the host's table [L][8] indexed by k = L - 1 - j: h[j], Re gz[j],
// Im gz[j], Re gp[j], Im gp[j] (gz, gp: the complex taps of ldsp.h), the bits of
// stbank_slot(D, L, k) and two words of padding.  thr2: the float32 square of
// the pilot threshold.  y[(2 c) * ldy + m] receives row c's left,
// y[(2 c + 1) * ldy + m] its right; level[c] receives sqrtf(|P|^2) of the call's
// last column (untouched by a call without columns).  n = 0 launches nothing.
constexpr int kStbankMaxC = 128;
constexpr int kStbankMaxD = 32;
constexpr int kStbankMaxL = 1025;
int stbank_frames(int D, int L);                            // output columns per workgroup
int stbank_slot(int D, int L, int k);                       // where the staged span keeps offset k of column 0
struct StbankCall {
    const float* x;
    const float* hist;
    float* hist_out;
    size_t n, ldx, skip, ncols, ldy;
    int C, D, L;
    const float* taps;
    float thr2;
    float* y;
    float* level;
};
void stbank(const StbankCall& c, hipStream_t s);
// k_ambank.hip: coherent AM demodulator over bank rows (AMBank).  C <= kAmbankMaxC
// rows of complex64, row c's n samples at x + c * ldx (in samples); decimation
// 1 <= D <= kAmbankMaxD, two real prototypes of L <= kAmbankMaxL taps.  hist /
// hist_out: per row the L - 1 raw samples before x[c][0] / before the next
// call's first, [C][L - 1] complex64, distinct buffers (at least one readable
// sample when L = 1).  The call's columns are at sample skip + m D, m < ncols, as
// k_chan's.  taps: the host's table [L][4] indexed by k = L - 1 - j: d[j], g[j]
// (ldsp.h), the bits of ambank_slot(D, L, k) and one word of padding.  thr2: the
// float32 square of the carrier threshold.  y[c * ldy + m] receives row c's
// output; level[c] receives sqrtf(|Cr|^2) of the call's last column (untouched
// by a call without columns).  n = 0 launches nothing.
constexpr int kAmbankMaxC = 256;
constexpr int kAmbankMaxD = 32;
constexpr int kAmbankMaxL = 1025;
int ambank_frames(int D, int L);                            // output columns per workgroup
int ambank_slot(int D, int L, int k);                       // where the staged span keeps offset k of column 0, in pairs
struct AmbankCall {
    const void* x;
    const void* hist;
    void* hist_out;
    size_t n, ldx, skip, ncols, ldy;
    int C, D, L;
    const float* taps;
    float thr2;
    float* y;
    float* level;
};
void ambank(const AmbankCall& c, hipStream_t s);
// k_ssbbank.hip: tuned single-sideband demodulator over bank rows (SSBBank).
// C <= kSsbbankMaxC rows of complex64, row c's n samples at x + c * ldx (in
// samples); decimation 1 <= D <= kSsbbankMaxD, per row L <= kSsbbankMaxL complex
// taps.  hist / hist_out: per row the L - 1 raw samples before x[c][0] / before
// the next call's first, [C][L - 1] complex64, distinct buffers (at least one
// readable sample when L = 1).  The call's columns are at sample skip + m D,
// m < ncols, as k_chan's; col0 is the absolute index of column m = 0 (the
// rotation's).  taps: the host's table [C][L][4] indexed by k = L - 1 - j:
// Re g_c[j], Im g_c[j] (ldsp.h), the bits of ssbbank_slot(D, L, k) and one word
// of padding.  words: the C 32-bit BFO words.  y[c * ldy + m] receives row c's
// output.  n = 0 launches nothing.
constexpr int kSsbbankMaxC = 256;
constexpr int kSsbbankMaxD = 32;
constexpr int kSsbbankMaxL = 1025;
int ssbbank_frames(int D, int L);                           // output columns per workgroup
int ssbbank_slot(int D, int L, int k);                      // where the staged span keeps offset k of column 0, in pairs
struct SsbbankCall {
    const void* x;
    const void* hist;
    void* hist_out;
    size_t n, ldx, skip, ncols, ldy;
    unsigned long long col0;
    int C, D, L;
    const float* taps;
    const uint32_t* words;
    float* y;
};
void ssbbank(const SsbbankCall& c, hipStream_t s);
// k_synth.hip: polyphase synthesis filter bank (Synthesizer), k_chan's
// counterpart.  M rows (a power of two, 4 .. 256), interpolation D = M or M / 2,
// Q = ceil(L / D) <= synth_qmax(M, D) taps per output residue.  y: row k at
// y + k * ld, ncols columns of complex64; hist / hist_out: the Q - 1 columns
// before the call's first / before the next call's first as [M][Q - 1],
// distinct buffers (at least one readable sample when Q = 1); taps: the
// prototype zero-padded to kChanMaxP * M floats; tw as k_chan's; parity: that of
// the first column's absolute index (the D = M / 2 sign).  z receives
// ncols * D samples.  ncols = 0 launches nothing.
constexpr int synth_qmax(int M, int D) { return kChanMaxP * (M / D); }
constexpr int synth_cols(int M) { return chan_frames(M); }            // input columns per workgroup
struct SynthCall {
    const void* y;
    const void* hist;
    void* hist_out;
    size_t ncols, ld;
    int parity, Q;
    const float* taps;
    const void* tw;
    float scale;
    void* z;
};
void synth(int M, int D, const SynthCall& c, hipStream_t s);
// k_spgram.hip: streaming Welch periodogram (Spectrogram).  N = nfft (a power of
// two, 256 .. 4096), window of W <= N taps, hop d <= W, A transforms per row.
// x: n complex64 samples; hist / hist_out: the W - 1 samples before x[0] / before
// the next call's x[0], distinct buffers; win: the window zero-padded to N
// floats; tw[j] = exp(-2 pi i j / N), j < N.  The call takes nt transforms, the
// first with its window starting at x[base] (base > -W), the next ones d samples
// on; a0 of the first row's A transforms were taken by earlier calls, whose sum
// is carry_in (float32[N]); a row the call does not finish leaves its sum in
// carry_out (a distinct buffer).  Finished row r of the call, times scale, goes to y + r * ld
// (y may be NULL: nothing is stored); every transform is added to psd (float64[N])
// by way of part, room for spgram_runs() * N floats.  n = 0 launches nothing.
constexpr int kSpgramMaxRuns = 2048;                  // workgroups of one call at the most
constexpr int spgram_tile(int N) { return N >= 2048 ? 8 : 16384 / N; }   // transforms per workgroup
struct SpgramCall {
    const void* x;
    const void* hist;
    void* hist_out;
    size_t n, A, a0, nt, ld;
    long long base;
    int W, d;
    const float* win;
    const void* tw;
    const float* carry_in;
    float* carry_out;
    float scale;          // of a finished row's sum: 1 / A (1 for the block sums of a blocked average)
    float* y;
    float* part;
    double* psd;
    bool iq16 = false;
};
// workgroups (runs of whole rows) a call of nt transforms is cut into: rows of
// spgram_tile(N) transforms together, more when that would pass kSpgramMaxRuns
size_t spgram_runs(int N, size_t A, size_t a0, size_t nt, size_t* rows_per_run);
void spgram(int N, const SpgramCall& c, hipStream_t s);
// Blocked averages: A a multiple of kSpgramBlock and at least twice it.  spgram()
// then runs with A = kSpgramBlock and y = blk (ld = N, nb finished blocks), and
// spgram_rows adds the blocks of each row (M = A / kSpgramBlock of them, c0 of the
// first row's taken by earlier calls and summed in carry_in) into y + r * ld, or
// into carry_out for the row the call does not finish.  At most
// kSpgramMaxBlocks / M + 1 rows per launch.
constexpr int kSpgramBlock = 8;
constexpr size_t kSpgramMaxBlocks = 16384;            // finished blocks of one spgram() + spgram_rows() pair
constexpr bool spgram_blocked(size_t A) { return A >= 2 * kSpgramBlock && A % kSpgramBlock == 0; }
void spgram_rows(int N, const float* blk, size_t nb, size_t M, size_t c0, const float* carry_in, float* carry_out,
                 size_t A, float* y, size_t ld, hipStream_t s);
struct FmState {          // FMStereo mixer loop state (device-resident)
    uint32_t theta, dtheta;
    float pe, alpha, beta;
};
void fm_pll(const float* s, size_t n, FmState* st, const float* table, float* l, float* r, hipStream_t strm);
void interleave2(const float* a, const float* b, size_t n, float* y, hipStream_t strm);

} // namespace k
} // namespace ldsp
