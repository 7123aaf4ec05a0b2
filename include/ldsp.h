/*
 * ldsp.h -- C ABI of libldsp, the MI355X (gfx950) streaming-DSP library that
 * replaces the liquid-dsp calls behind python-liquiddsp's hot path.
 *
 * Every entry point below names the reference interface it replaces
 * (colbyAtCRI/python-liquiddsp, paths relative to the repository root) and the
 * liquid-dsp routine that interface calls.  The pybind11 module `liquiddsp`
 * (python-liquiddsp_amd/pybind/liquiddsp_module.cpp) binds these with the same
 * class names, keyword arguments and properties as src/wrapper.cpp; a ctypes or
 * other FFI binding can call them directly.
 *
 * Conventions
 *  - All functions return LDSP_OK (0) or a negative LDSP_E* code; the message
 *    of the last failure on the calling thread is ldsp_last_error().
 *  - Handles are independent; calls on one handle must not overlap in time and
 *    must be issued on one stream (or be externally ordered).
 *  - Sample buffers: complex samples are interleaved float32 (re, im) =
 *    numpy.complex64; real samples float32.  `mem` says whether x / y are host
 *    pointers (LDSP_MEM_HOST: the call stages through the device and returns
 *    after the result is in y) or device pointers (LDSP_MEM_DEVICE: the call
 *    only enqueues work on `stream` (a hipStream_t, NULL = default stream) and
 *    returns immediately).
 *  - Streaming state (filter history, resampler / NCO phase, IIR state, AGC
 *    gain, PLL) lives in device memory owned by the handle and carries across
 *    calls exactly like the liquid objects' internal state.
 *  - Objects can be created and configured without a GPU (design, properties,
 *    freqresponse are host-side); device memory is allocated on first execute.
 */
#ifndef LDSP_H
#define LDSP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LDSP_OK      0
#define LDSP_EINVAL (-1)   /* invalid configuration / argument (Python ValueError) */
#define LDSP_ENOMEM (-2)   /* allocation failure */
#define LDSP_EHIP   (-3)   /* HIP runtime failure or no GPU (Python RuntimeError) */
#define LDSP_ERANGE (-4)   /* output capacity too small */
#define LDSP_EUNSUP (-5)   /* configuration not implemented */

#define LDSP_MEM_HOST   0
#define LDSP_MEM_DEVICE 1

/* execution modes (exact = bit-identical to the sequential CPU restatement) */
#define LDSP_MODE_FAST  0
#define LDSP_MODE_EXACT 1
#define LDSP_MODE_DIRECT 2   /* FIR only: fast direct form (bitwise invariant to how a stream is cut into calls) */

const char *ldsp_last_error(void);
int ldsp_version(void);
int ldsp_device_count(int *n);
int ldsp_stream_synchronize(void *stream);

/* Page-locked host buffers for LDSP_MEM_HOST calls (no reference counterpart:
 * the reference returns pageable numpy arrays from every __call__,
 * src/firfilter.hpp:25-35, src/iirfilter.hpp:292-298, src/resampler.hpp:144-152).
 * An LDSP_MEM_HOST call whose x or y lies in page-locked memory (from here, or
 * hipHostMalloc / hipHostRegister) copies it by DMA directly instead of through
 * the library's staging buffer, so a chain of host calls that hands one call's
 * output to the next skips two host copies per hand-over.  Blocks are pooled:
 * ldsp_host_free keeps up to 256 MB of them for reuse.  ldsp_host_alloc fails
 * with LDSP_ENOMEM once 1 GB is handed out (callers then use pageable memory). */
int ldsp_host_alloc(size_t bytes, void **p);
int ldsp_host_free(void *p);

/* Test hook: the per-thread staging pools of LDSP_MEM_HOST calls.  A thread
 * takes one pool per device on its first host call and returns it to a
 * process-wide free list when it exits, so *total (pools ever created) stays at
 * the number of threads making host calls concurrently; *idle = pools on the
 * free list. */
int ldsp_debug_host_pools(size_t *total, size_t *idle);

/* Test hook: evaluate the loop transcendentals (ldsp_math.hpp) on the device.
 * fn: 0 exp, 1 log, 2 atan2(a, b), 3 tanh, 4 constrain (y as uint32 bits);
 * 5 exp, 6 log through the loops' fast paths (lm_*_loop); 7 atan2(a, b) in its
 * select-only form (lm_atan2f_vsel: the candidate evaluations of k_pll_seqc and
 * k_fm_pll); 8 constrain through v_fract (lm_constrain_fr: k_fm_pll's chain).
 * a, b, y are device pointers of n floats. */
int ldsp_debug_math_eval(int fn, const float *a, const float *b, float *y, size_t n, void *stream);

/* Test hook (host only, no device): check the loops' fast paths (ldsp_math.hpp
 * lm_logf_fast, lm_expf_fast) against the general functions on every stride-th
 * float bit pattern in [begin, end) that lies in the fast range (fn 0 log,
 * 1 exp).  *checked: patterns in the fast range; *mismatches: how many differ in
 * any bit. */
int ldsp_debug_math_fastcheck(int fn, uint32_t begin, uint32_t end, uint32_t stride, uint64_t *checked,
                              uint64_t *mismatches);

/* Per-kernel device timing (no reference counterpart; measurement support for
 * bench.py).  While enabled every kernel launch is bracketed by a HIP event
 * pair on its stream; the report lists "name calls total_ms" lines. */
int ldsp_profile_enable(int on);
int ldsp_profile_reset(void);
/* time only the launches of the kernel named `kernel` (NULL or "": every kernel) */
int ldsp_profile_only(const char *kernel);
int ldsp_profile_report(char *buf, size_t cap, size_t *len);

/* ------------------------------------------------------------------------
 * FIR filter: firfilt_rrrf (cplx=0) / firfilt_crcf (cplx=1), real taps.
 * Replaces RealFIRFilter (src/firfilter.hpp:13-35, firfilt_rrrf_create /
 * firfilt_rrrf_execute_block), RealDCBlocker (firfilter.hpp:42-44,
 * firfilt_rrrf_create_dc_blocker), RealKaiserBessel (firfilter.hpp:56-61,
 * firfilt_rrrf_create_kaiser + set_scale) and the crcf filter used inside
 * demod.hpp:105,135-136 (new class ComplexFIRFilter).
 * ---------------------------------------------------------------------- */
typedef struct ldsp_firfilt_s *ldsp_firfilt_t;
int ldsp_firfilt_create(const float *h, unsigned int n, int cplx, ldsp_firfilt_t *q);
int ldsp_firfilt_create_kaiser(unsigned int n, float fc, float as, float mu, int cplx, ldsp_firfilt_t *q);
int ldsp_firfilt_create_dc_blocker(unsigned int m, float as, int cplx, ldsp_firfilt_t *q);
int ldsp_firfilt_destroy(ldsp_firfilt_t q);
int ldsp_firfilt_reset(ldsp_firfilt_t q);
int ldsp_firfilt_set_scale(ldsp_firfilt_t q, float scale);
int ldsp_firfilt_get_scale(ldsp_firfilt_t q, float *scale);
int ldsp_firfilt_get_length(ldsp_firfilt_t q, unsigned int *n);
int ldsp_firfilt_get_taps(ldsp_firfilt_t q, float *h);
/* mode: LDSP_MODE_FAST (default; complex data with 48 <= L <= 513 taps uses
 * overlap-save FFT convolution, HBM-bound), LDSP_MODE_DIRECT (register-blocked
 * direct form), LDSP_MODE_EXACT (liquid dot-product order, bit-identical). */
int ldsp_firfilt_set_mode(ldsp_firfilt_t q, int mode);
int ldsp_firfilt_get_mode(ldsp_firfilt_t q, int *mode);
/* Test hook, host logic only (works without a GPU): the kernel the next call of
 * n samples runs -- 0 direct form, 1 overlap-save FFT, 2 exact -- and, for the
 * FFT, its window length (512 / 1024 points) and the overlap P (history samples
 * per window, a multiple of 64; the hop is points - P).  Pointers may be NULL. */
int ldsp_debug_fir_dispatch(ldsp_firfilt_t q, size_t n, int *kernel, int *points, int *overlap);
/* firfilt_*_freqresponse (firfilter.hpp:23-27) */
int ldsp_firfilt_freqresponse(ldsp_firfilt_t q, float f, float *re, float *im);
/* firfilt_*_execute_block (firfilter.hpp:29-35): y[i] = scale * sum_k h[k] x[i-k] */
int ldsp_firfilt_execute(ldsp_firfilt_t q, const void *x, size_t n, void *y, int mem, void *stream);

/* ------------------------------------------------------------------------
 * Arbitrary-rate polyphase resampler: resamp_rrrf (cplx=0) / resamp_cccf
 * (cplx=1).  Replaces RealResampler / ComplexResampler
 * (src/resampler.hpp:72-173: resamp_*_create(rate, m, fc, As, npfb),
 * resamp_*_execute per sample, set_rate, reset, print).
 * ---------------------------------------------------------------------- */
typedef struct ldsp_resamp_s *ldsp_resamp_t;
/* cplx: 0 resamp_rrrf, 1 resamp_cccf (ComplexResampler), 2 resamp_crcf (complex
 * samples, real taps: CResampler) */
int ldsp_resamp_create(float rate, unsigned int m, float fc, float as, unsigned int npfb, int cplx,
                       ldsp_resamp_t *q);
/* resamp_*_create_default(rate): RResampler / CResampler (src/resampler.hpp:10-13,
 * 46-49; wrapper.cpp:15-23).  m = 7, fc = 0.25, As = 60, npfb = 256 (liquid-dsp
 * resamp.proto.c defaults, recalled: parity unpinned). */
int ldsp_resamp_create_default(float rate, int kind, ldsp_resamp_t *q);
int ldsp_resamp_destroy(ldsp_resamp_t q);
int ldsp_resamp_reset(ldsp_resamp_t q);
int ldsp_resamp_set_rate(ldsp_resamp_t q, float rate);
int ldsp_resamp_get_rate(ldsp_resamp_t q, float *rate);
/* npfb (after power-of-two rounding), step, current phase, taps per branch */
int ldsp_resamp_get_info(ldsp_resamp_t q, unsigned int *npfb, uint32_t *step, uint32_t *phase,
                         unsigned int *sub_len);
int ldsp_resamp_get_taps(ldsp_resamp_t q, float *h, unsigned int cap, unsigned int *n);
/* number of outputs the next execute of n inputs will produce (host-side, exact) */
int ldsp_resamp_num_outputs(ldsp_resamp_t q, size_t n, size_t *nout);
int ldsp_resamp_execute(ldsp_resamp_t q, const void *x, size_t n, void *y, size_t cap, size_t *nout,
                        int mem, void *stream);
/* Test hook, host logic only (works without a GPU): the kernel the next call of
 * n samples runs at the current phase -- 0 tile (taps and span in LDS), 1 direct
 * (branch table in LDS, windows from global memory), 2 staged (span in LDS, taps
 * from global memory; also every call without outputs) -- and its outputs per
 * workgroup.  Pointers may be NULL. */
int ldsp_debug_resamp_dispatch(ldsp_resamp_t q, size_t n, int *kernel, int *outputs_per_group);

/* ------------------------------------------------------------------------
 * NCO: nco_crcf (type 0 = LIQUID_NCO table, 1 = LIQUID_VCO).  Replaces NCO
 * (src/nco.hpp:4-81): frequency / phase accessors, PLL helpers and
 * nco_crcf_mix_block_up / _down (nco.hpp:66-80).
 * ---------------------------------------------------------------------- */
typedef struct ldsp_nco_s *ldsp_nco_t;
int ldsp_nco_create(int type, ldsp_nco_t *q);
int ldsp_nco_destroy(ldsp_nco_t q);
int ldsp_nco_reset(ldsp_nco_t q);
int ldsp_nco_set_frequency(ldsp_nco_t q, float f);
int ldsp_nco_get_frequency(ldsp_nco_t q, float *f);
int ldsp_nco_adjust_frequency(ldsp_nco_t q, float df);
int ldsp_nco_set_phase(ldsp_nco_t q, float phi);
int ldsp_nco_get_phase(ldsp_nco_t q, float *phi);
int ldsp_nco_adjust_phase(ldsp_nco_t q, float dphi);
int ldsp_nco_pll_set_bandwidth(ldsp_nco_t q, float bw);
int ldsp_nco_pll_step(ldsp_nco_t q, float dphi);
int ldsp_nco_get_state(ldsp_nco_t q, uint32_t *theta, uint32_t *dtheta);
int ldsp_nco_set_state(ldsp_nco_t q, uint32_t theta, uint32_t dtheta);
int ldsp_nco_mix(ldsp_nco_t q, const void *x, size_t n, void *y, int down, int mem, void *stream);

/* NCO mix fused into a complex FIR: y = fir(nco.mix_down(x)) (down = 1) or
 * fir(nco.mix_up(x)), the chain of BASELINE config 3 (reference src/nco.hpp:74-80
 * NCO::mix_down, then src/firfilter.hpp:29-35 execute_block).  Advances the NCO
 * phase by n * dtheta and the filter's history exactly as ldsp_nco_mix followed
 * by ldsp_firfilt_execute would, with the same output bits; on the filter's
 * overlap-save path (fast mode, table NCO) the mixed samples are formed as the
 * filter loads x and never reach memory (16 B per sample instead of 32).  The
 * filter must be complex (firfilt_crcf); both objects on the buffer's device. */
int ldsp_nco_mix_firfilt(ldsp_nco_t nco, ldsp_firfilt_t fir, const void *x, size_t n, void *y, int down, int mem,
                         void *stream);

/* ------------------------------------------------------------------------
 * IIR filter: iirfilt_rrrf (cplx=0) / iirfilt_crcf (cplx=1).  Replaces
 * ComplexIIRFilter / RealIIRFilter (src/iirfilter.hpp:243-356,
 * iirfilt_*_create_prototype(..., LIQUID_IIRDES_SOS, ...)), the
 * C/R{Lowpass,Highpass,Bandpass,Bandstop}IIR family (iirfilter.hpp:61-241),
 * CIIRFilter / RIIRFilter raw transfer functions (iirfilter.hpp:30-34,140-144,
 * iirfilt_*_create) and DeemphasisFilter (iirfilter.hpp:358-392).
 * ftype: 0 butter 1 cheby1 2 cheby2 3 ellip 4 bessel;
 * btype: 0 lowpass 1 highpass 2 bandpass 3 bandstop.
 * Mode FAST evaluates the cascade as a chunked linear scan in float64 (more
 * accurate than liquid's float32 recursion): in one pass over memory in the
 * filter's modal coordinates when they are well-conditioned, else as a blocked
 * scan of the SOS state; EXACT runs the float32 direct-form II recursion
 * (bit-identical to the restatement): sequentially, or -- for filters that
 * forget their state within 16 384 samples (de-emphasis, DC blockers) -- as
 * speculative chunks started early from zero whose start states a verifier
 * checks bit for bit against their predecessors' (the same bits).  Fast mode
 * takes that path for those filters too.
 * ---------------------------------------------------------------------- */
typedef struct ldsp_iirfilt_s *ldsp_iirfilt_t;
int ldsp_iirfilt_create_prototype(int ftype, int btype, unsigned int order, float fc, float f0,
                                  float ap, float as, int cplx, ldsp_iirfilt_t *q);
int ldsp_iirfilt_create_sos(const float *B, const float *A, unsigned int nsos, int cplx,
                            ldsp_iirfilt_t *q);
int ldsp_iirfilt_create_tf(const float *b, unsigned int nb, const float *a, unsigned int na, int cplx,
                           ldsp_iirfilt_t *q);
/* Test / diagnostic hooks for the fast-mode evaluation.  The fast mode runs the
 * single-pass modal scan (k_iir_modal) when the filter's modal form passed its
 * host check at creation (ok = 1: modes M, look-back depth J in 2048-sample
 * units, check error err), else the blocked SOS-coordinate scan.  path: 0
 * automatic, 1 force the blocked scan, 2 require the modal scan (LDSP_EINVAL
 * when the filter has none), 3 the modal scan with every look-back recomputed
 * from the input (the path a wave takes when a predecessor is late).  A forced
 * path also replaces the speculative exact path of fast-decaying filters;
 * exact mode is unaffected. */
int ldsp_debug_iir_path(ldsp_iirfilt_t q, int path);
/* Diagnostics, no reference counterpart: while dev_buf (device memory, at least
 * objects x 2 x 9 x 4 uint64) is set, every exact SOS launch (k_iir_sect)
 * writes per (object, component, section wave) the shader clocks spent waiting
 * for its input / ring space, forming its input tile, in its recursion, and in
 * all.  NULL turns it off.  Not thread-safe; for timing studies. */
int ldsp_debug_iir_sect_trace(void *dev_buf);
int ldsp_debug_iir_modal_info(ldsp_iirfilt_t q, int *ok, int *modes, int *lookback, double *err);
/* Test hook, host logic only: the grid of a modal-scan call of n samples --
 * its 2048-sample units, whether it runs in the one-XCD small-call mode
 * (units <= 16 x look-back) and the workgroups launched (8 x units in that
 * mode, else units).  A many-call merges modal launches of equal grid, and only
 * grids that are a multiple of 8.  Pointers may be NULL. */
int ldsp_debug_iir_modal_grid(ldsp_iirfilt_t q, size_t n, long *units, int *one_xcd, unsigned int *grid);
/* Test hook, host logic only (works without a GPU): what a call of n samples
 * runs with the current mode and forced path.  path: 0 speculative exact chunks,
 * 1 sequential exact, 2 modal scan, 3 blocked scan (D <= 8), 4 chunked scan.
 * sect_tile: on the sequential path, the tile of k_iir_sect (512 / 1024) or 0
 * for k_iir_seq.  size_class: the unroll class (2, 4 or 17 sections /
 * coefficients) of k_iir_seq and of the speculative kernels.  spec_W: the
 * filter's warm-up length (0: it does not forget its state within 4096
 * samples).  spec_staged: 1 when the speculative chunk kernel stages its input
 * window in LDS.  Pointers may be NULL. */
int ldsp_debug_iir_dispatch(ldsp_iirfilt_t q, size_t n, int *path, int *sect_tile, int *size_class, int *spec_W,
                            int *spec_staged);
int ldsp_iirfilt_destroy(ldsp_iirfilt_t q);
int ldsp_iirfilt_reset(ldsp_iirfilt_t q);
int ldsp_iirfilt_set_mode(ldsp_iirfilt_t q, int mode);
int ldsp_iirfilt_get_nsos(ldsp_iirfilt_t q, unsigned int *nsos);
int ldsp_iirfilt_get_sos(ldsp_iirfilt_t q, float *B, float *A);
int ldsp_iirfilt_freqresponse(ldsp_iirfilt_t q, float f, float *re, float *im);
int ldsp_iirfilt_execute(ldsp_iirfilt_t q, const void *x, size_t n, void *y, int mem, void *stream);
/* bytes_to_iq fused into the filter (replaces the pair
 * `filter(bytes_to_iq(raw))`, src/utility.hpp:61-69 + iirfilter.hpp:292-298):
 * x holds n native int16 (I, Q) pairs (4 n bytes), each converted to
 * (float)v / 32767.0f exactly as bytes_to_iq does; y receives n complex64
 * outputs, the same bits as ldsp_bytes_to_iq followed by ldsp_iirfilt_execute.
 * Complex filters only (LDSP_EINVAL otherwise).  The blocked float64 scan (the
 * default fast mode) converts on load, so the input is read at 4 B per sample;
 * the exact and speculative paths convert with one extra pass first. */
int ldsp_iirfilt_execute_iq16(ldsp_iirfilt_t q, const void *x, size_t n, void *y, int mem, void *stream);
/* resamp(iirfilt(x)) in one call: the chain's first two stages (reference
 * README.md:53-54, src/iirfilter.hpp:292-298 then src/resampler.hpp:160-172;
 * an opt-in fusion, not a reference entry point).  y receives the resampler's
 * outputs (*nout = ldsp_resamp_num_outputs(rs, n), at most cap), the same bits
 * and the same state updates of both objects as ldsp_iirfilt_execute into a
 * scratch buffer followed by ldsp_resamp_execute on it.  When the filter takes
 * the modal scan (fast mode) the filter outputs never reach HBM; otherwise the
 * two calls run.  Both objects complex (complex64) or both real. */
int ldsp_iirfilt_resamp_execute(ldsp_iirfilt_t q, ldsp_resamp_t rs, const void *x, size_t n, void *y, size_t cap,
                                size_t *nout, int mem, void *stream);

/* ------------------------------------------------------------------------
 * AGC: agc_crcf.  Replaces AGC (src/agc.hpp:4-149).  execute implements
 * AGC::execute (agc.hpp:109-128): agc_crcf_execute per sample, squelch status
 * polled per sample, output zeroed in SIGNALLO / ENABLED.  When `status` is
 * non-NULL it receives the per-sample squelch status (host array of n bytes;
 * the call then synchronises) so the caller can replay onRise callbacks.
 * ---------------------------------------------------------------------- */
typedef struct ldsp_agc_s *ldsp_agc_t;
int ldsp_agc_create(ldsp_agc_t *q);
/* Test hook: small AGC calls (the one-wave chunk path, 320 <= n < the
 * chunk-parallel threshold) start every chunk but the first 1 ulp away from its
 * approximated state, so the in-kernel check re-runs each of them from its
 * predecessor's end state; the output stays bit-identical to agc_crcf. */
int ldsp_debug_agc_tsa_perturb(ldsp_agc_t q, int on);
/* chunks re-run by that in-kernel check since the object was created */
int ldsp_debug_agc_tsa_reruns(ldsp_agc_t q, unsigned int *count);
/* Test hooks for chunk-parallel calls (above the small-call range): with
 * perturb on, every odd chunk starts from its guessed state with the gain 1 ulp
 * off, so the flag pass marks it and the repair rounds / the verifier re-run it
 * from its predecessor's true end state (output still bit-identical to
 * agc_crcf).  rounds: parallel repair rounds before the one-wave verifier (-1 =
 * the default, 1; 0 = the verifier alone re-runs every flagged chunk).
 * reruns: chunks re-run since the object was created, by the repair rounds
 * (*runfix) and by the verifier (*verify). */
int ldsp_debug_agc_perturb(ldsp_agc_t q, int on);
int ldsp_debug_agc_rounds(ldsp_agc_t q, int rounds);
int ldsp_debug_agc_reruns(ldsp_agc_t q, unsigned int *runfix, unsigned int *verify);
/* Test hook, host logic only (works without a GPU): the path the next call of n
 * samples takes, from the function ldsp_agc_execute itself decides with --
 * *path 0 the sequential loop, 1 small-call chunks from the true state, 2
 * chunk-parallel; the warm-up lengths W (exact) and Wa (approximate) of the
 * current bandwidth; the chunk length C (0 on path 0); the input history a
 * speculative call needs (W + Wa + 256) and how much of it the object holds;
 * *spec 1 when the call runs from the history alone (front, repair, verify
 * launches instead of front, back).  Pointers may be NULL. */
int ldsp_debug_agc_dispatch(ldsp_agc_t q, size_t n, int *path, int *W, int *Wa, int *C, long *hist_len,
                            long *hist_valid, int *spec);
int ldsp_agc_destroy(ldsp_agc_t q);
int ldsp_agc_reset(ldsp_agc_t q);
int ldsp_agc_set_bandwidth(ldsp_agc_t q, float bw);
int ldsp_agc_get_bandwidth(ldsp_agc_t q, float *bw);
int ldsp_agc_lock(ldsp_agc_t q, int on);
int ldsp_agc_squelch_enable(ldsp_agc_t q, int on);
int ldsp_agc_squelch_set_threshold(ldsp_agc_t q, float t);
int ldsp_agc_squelch_get_threshold(ldsp_agc_t q, float *t);
int ldsp_agc_squelch_set_timeout(ldsp_agc_t q, unsigned int t);
int ldsp_agc_squelch_get_status(ldsp_agc_t q, int *status);
int ldsp_agc_get_gain(ldsp_agc_t q, float *g);
int ldsp_agc_set_gain(ldsp_agc_t q, float g);
int ldsp_agc_get_scale(ldsp_agc_t q, float *s);
int ldsp_agc_set_scale(ldsp_agc_t q, float s);
int ldsp_agc_get_signal_level(ldsp_agc_t q, float *x);
int ldsp_agc_set_signal_level(ldsp_agc_t q, float x);
int ldsp_agc_get_rssi(ldsp_agc_t q, float *r);
int ldsp_agc_set_rssi(ldsp_agc_t q, float r);
int ldsp_agc_set_mode(ldsp_agc_t q, int mode);
int ldsp_agc_execute(ldsp_agc_t q, const void *x, size_t n, void *y, uint8_t *status, int mem,
                     void *stream);

/* ------------------------------------------------------------------------
 * AM demodulator: ampmodem (type 0 dsb, 1 usb, 2 lsb).  Replaces AmpModem
 * (src/demod.hpp:221-307: ampmodem_create(mod, type, suppressed_carrier),
 * ampmodem_demodulate_block, ampmodem_reset).  dsb: carrier PLL (carrier) or
 * Costas loop (suppressed); usb / lsb: the carrier PLL then a Hilbert c2r
 * (carrier), or the Hilbert c2r alone (suppressed).
 * ---------------------------------------------------------------------- */
typedef struct ldsp_ampmodem_s *ldsp_ampmodem_t;
int ldsp_ampmodem_create(float mod_index, int type, int suppressed_carrier, ldsp_ampmodem_t *q);
int ldsp_ampmodem_destroy(ldsp_ampmodem_t q);
int ldsp_ampmodem_reset(ldsp_ampmodem_t q);
int ldsp_ampmodem_get_pll_state(ldsp_ampmodem_t q, uint32_t *theta, uint32_t *dtheta);
/* The designs inside (liquid ampmodem_create): carrier lowpass (2m+1 = 51 taps,
 * firfilt_crcf_create_kaiser(51, 0.01, 40, 0)), DC blocker (51 taps,
 * firfilt_rrrf_create_dc_blocker(25, 20)) and the usb / lsb Hilbert transform's
 * 2m = 50 quadrature taps (firhilbf_create(25, 60), see firhilb.proto.c).  Any
 * pointer may be NULL.  Host only. */
int ldsp_ampmodem_get_taps(ldsp_ampmodem_t q, float *lowpass, float *dcblock, float *hilbert);
int ldsp_ampmodem_demodulate(ldsp_ampmodem_t q, const void *x, size_t n, void *y, int mem,
                             void *stream);
/* Diagnostics, no reference counterpart: the exact PLL walk of the last call
 * that ran chunk-parallel (k_pll.hip) -- entries visited, repairs (samples
 * whose true table index differed from the candidate's) and lane-blocks redone
 * sample by sample.  All zero after a sequential (short) call.  Synchronises. */
int ldsp_ampmodem_walk_stats(ldsp_ampmodem_t q, uint64_t *entries, uint64_t *repairs,
                             uint64_t *fallbacks);
/* Diagnostics, no reference counterpart: the carrier-mode short-call loop
 * (k_pll_seqc, calls below 2 048 samples), cumulative since the object's first
 * call: candidate batches stepped and batches redone directly because a table
 * index left its candidate window.  Synchronises. */
int ldsp_ampmodem_seq_stats(ldsp_ampmodem_t q, uint64_t *batches, uint64_t *redone);
/* Diagnostics, no reference counterpart: walker clock counters of the last
 * chunk-parallel call (shader clocks spent walking / waiting at the per-block
 * barrier), written only by the timing variants of a tuning build (zero
 * otherwise).  Synchronises. */
int ldsp_ampmodem_walk_clocks(ldsp_ampmodem_t q, uint64_t *walk, uint64_t *wait);
/* Diagnostics, no reference counterpart: the chunk-parallel walker's active time,
 * cumulative since the object was created -- 10 ns ticks from the moment a walk
 * has the previous call's state (a walker may be dispatched before that and wait
 * on the device) to its end, and the number of walks.  Raises LDSP_EHIP if a
 * walker's wait timed out.  Synchronises. */
int ldsp_ampmodem_walk_active(ldsp_ampmodem_t q, uint64_t *ticks, uint64_t *count);
/* Diagnostics, no reference counterpart: the walker's entry margin B = 2^log2_b
 * for the calls that follow (8..21; 0 restores the default).  A narrower
 * margin leaves fewer entries and fails more gap proofs, so more lane-blocks
 * are redone sample by sample -- the tests use it to exercise that path.
 * Returns the previous setting. */
int ldsp_debug_pll_margin(int log2_b);
/* Test hook, no reference counterpart, needs no GPU: the interval fields of one
 * walker entry record as the entry kernel computes them (the same inline function).
 * u: position in the table cell (22 bits); margin B; left_gap / right_gap: the gap
 * to the previous / next entry is non-empty; dk2: a repair's step.  out[0..3] =
 * lo (as uint32), W, amin, awidth: with x = f - lo, no event iff x <=u W, and the
 * walker's test over all lanes passes iff x <=u W or x - amin <=u awidth. */
int ldsp_debug_walk_fold(uint32_t u, int32_t b, int left_gap, int right_gap, uint32_t dk2, uint32_t out[4]);
/* Test hook, no reference counterpart: the bound of an early-dispatched
 * walker's wait for the previous call's PLL state (10 ns ticks; 0 restores the
 * default 1 s), and a skew added to the epoch the object's next walker waits for
 * (a skew of 1 makes it wait for a launch that never comes, so it times out).
 * A timed-out walk raises LDSP_EHIP at the object's next call or state read
 * until ldsp_ampmodem_reset.  Synchronises. */
int ldsp_debug_ampmodem_handoff(ldsp_ampmodem_t q, uint64_t wait_ticks, int epoch_skew);
/* Test hook, host logic only (works without a GPU): *parallel 1 when a call of
 * n samples runs the chunk-parallel PLL (scan, candidates, walk), 0 for the
 * sequential loop (the threshold differs between carrier and Costas modems);
 * *batchable 1 when a many-call merges this object's launches (dsb), 0 when it
 * makes the whole many-call run object by object.  Pointers may be NULL. */
int ldsp_debug_ampmodem_dispatch(ldsp_ampmodem_t q, size_t n, int *parallel, int *batchable);
/* Diagnostics, no reference counterpart: the walker's early hand-off for the
 * calls that follow (1 on, the default; 0 off: every walker waits for the
 * previous walk in stream order, so a kernel trace's k_pll_walk duration is the
 * walk itself; -1 restores the default).  Returns the previous setting. */
int ldsp_debug_walk_early(int on);

/* ------------------------------------------------------------------------
 * Broadcast AM demodulator.  Replaces BroadcastAM (src/demod.hpp:93-153,
 * wrapper.cpp:259-262): carrier PLL (Kaiser lowpass 2m+1, wdelaycf(m), NCO
 * PLL bw 0.001) followed by a cheby2 SOS highpass DC blocker (order 3,
 * fc 20/48000, Ap 0.5, As 20).  The PLL stage is bit-exact; the DC blocker
 * runs in LDSP_MODE_FAST (fp64 scan) by default, LDSP_MODE_EXACT on request.
 * `pre` (optional, device-or-host like y) receives re(v1) before the blocker.
 * ---------------------------------------------------------------------- */
typedef struct ldsp_bcastam_s *ldsp_bcastam_t;
int ldsp_bcastam_create(unsigned int m, ldsp_bcastam_t *q);
int ldsp_bcastam_destroy(ldsp_bcastam_t q);
int ldsp_bcastam_reset(ldsp_bcastam_t q);
int ldsp_bcastam_set_mode(ldsp_bcastam_t q, int mode);
int ldsp_bcastam_get_mode(ldsp_bcastam_t q, int *mode);
int ldsp_bcastam_demodulate(ldsp_bcastam_t q, const void *x, size_t n, void *y, void *pre, int mem,
                            void *stream);

/* ------------------------------------------------------------------------
 * Frequency demodulator.  Replaces FreqDem (src/demod.hpp:189-219,
 * wrapper.cpp:183-187 -> freqdem_create(kf), freqdem_demodulate_block):
 * y[n] = cargf(conjf(x[n-1]) x[n]) / (2 pi kf), bit-exact.
 * ---------------------------------------------------------------------- */
typedef struct ldsp_freqdem_s *ldsp_freqdem_t;
int ldsp_freqdem_create(float kf, ldsp_freqdem_t *q);
int ldsp_freqdem_destroy(ldsp_freqdem_t q);
int ldsp_freqdem_reset(ldsp_freqdem_t q);
int ldsp_freqdem_get_kf(ldsp_freqdem_t q, float *kf);
int ldsp_freqdem_demodulate(ldsp_freqdem_t q, const void *x, size_t n, void *y, int mem, void *stream);

/* ------------------------------------------------------------------------
 * FM stereo receiver.  Replaces FMStereo (src/demod.hpp:4-85, wrapper.cpp:264-267):
 * freqdem(4) -> composite mixer loop (NCO, PLL bandwidth 0.1, one-pole phase
 * error) -> 75 us de-emphasis per channel -> resamp_rrrf_create_default
 * (pcm_rate / iq_rate) per channel; output interleaved (L, R) float32.
 * Bit-exact; the mixer loop is inherently sequential (one lane).  reset()
 * resets only the resamplers, like the reference.  pcm_rate > iq_rate is
 * LDSP_EUNSUP.  num_outputs counts floats (2 per output pair).
 * ---------------------------------------------------------------------- */
typedef struct ldsp_fmstereo_s *ldsp_fmstereo_t;
int ldsp_fmstereo_create(float iq_rate, float pcm_rate, ldsp_fmstereo_t *q);
int ldsp_fmstereo_destroy(ldsp_fmstereo_t q);
int ldsp_fmstereo_reset(ldsp_fmstereo_t q);
int ldsp_fmstereo_num_outputs(ldsp_fmstereo_t q, size_t n, size_t *nout);
int ldsp_fmstereo_get_state(ldsp_fmstereo_t q, uint32_t *theta, uint32_t *dtheta, float *pe);
int ldsp_fmstereo_execute(ldsp_fmstereo_t q, const void *x, size_t n, void *y, size_t cap, size_t *nout,
                          int mem, void *stream);

/* ------------------------------------------------------------------------
 * Sample delay line.  Replaces Delay (src/utility.hpp:5-57, wrapper.cpp:25-28):
 * separate real (wdelayf) and complex (wdelaycf) lines of nd, read-then-push,
 * i.e. y[n] = x[n - nd - 1].  set_delay re-creates (zeroes) both lines.
 * ---------------------------------------------------------------------- */
typedef struct ldsp_delay_s *ldsp_delay_t;
int ldsp_delay_create(unsigned int nd, ldsp_delay_t *q);
int ldsp_delay_destroy(ldsp_delay_t q);
int ldsp_delay_set_delay(ldsp_delay_t q, unsigned int nd);
int ldsp_delay_get_delay(ldsp_delay_t q, unsigned int *nd);
int ldsp_delay_execute(ldsp_delay_t q, const void *x, size_t n, int cplx, void *y, int mem, void *stream);

/* ------------------------------------------------------------------------
 * Hilbert transform (firhilbf).  Replaces SSBDemod (src/demod.hpp:155-187,
 * wrapper.cpp:269-272: firhilbf_create(25, 60) + firhilbf_c2r_execute, one
 * sideband kept) and HilbertTransform (src/utility.hpp:71-108, wrapper.cpp:174-176:
 * two firhilbf_create(m, As) objects, firhilbf_interp_execute for complex input
 * and firhilbf_decim_execute for real input).  Over the stream z = history ++
 * input (zero history after create / reset), with hq the 2m quadrature taps:
 *   q[n] = sum_j hq[j] s[n - 4m + 1 + 2j]   (float32, sequential, oldest first)
 *   R2C    float32[n]   -> complex64[n]     y[n] = (z[n - 2m], q[n]), s = z
 *   C2R    complex64[n] -> float32[n] (x2)  s = im z, d = re z:
 *                                           y0[n] = d[n - 2m] + q[n] (lower sideband),
 *                                           y1[n] = d[n - 2m] - q[n] (upper sideband)
 *   DECIM  float32[2K]  -> complex64[K]     y[k] = the R2C output at n = 2k + 1
 *   INTERP complex64[K] -> float32[2K]      y[2k] = im z[k - m],
 *                                           y[2k + 1] = sum_j hq[j] re z[k + 1 - 2m + j]
 * Bit-exact with the restatement.  op is fixed per object (liquid's four
 * functions share the object's windows, so the reference keeps one object per
 * direction).  n counts input samples.  C2R: either of y0 / y1 may be NULL, not
 * both; the other ops write y0 and y1 must be NULL.  m < 2, an unknown op and an
 * odd n for DECIM are LDSP_EINVAL (checked before any device work); m > 64 is
 * LDSP_EUNSUP.
 * ---------------------------------------------------------------------- */
typedef struct ldsp_firhilb_s *ldsp_firhilb_t;
enum { LDSP_HILB_R2C = 0, LDSP_HILB_C2R = 1, LDSP_HILB_DECIM = 2, LDSP_HILB_INTERP = 3 };
int ldsp_firhilb_create(unsigned int m, float as, int op, ldsp_firhilb_t *q);
int ldsp_firhilb_destroy(ldsp_firhilb_t q);
int ldsp_firhilb_reset(ldsp_firhilb_t q);
int ldsp_firhilb_get_taps(ldsp_firhilb_t q, float *hq);          /* 2m floats */
int ldsp_firhilb_execute(ldsp_firhilb_t q, const void *x, size_t n, void *y0, void *y1, int mem, void *stream);
/* Test hook: input samples per workgroup of op's kernel (calls cut around it cross a tile edge). */
int ldsp_debug_firhilb_tile(int op, size_t *samples);

/* ------------------------------------------------------------------------
 * Channelizer: a polyphase analysis filter bank, one wideband complex64
 * stream to M channel rows in one pass.  No reference counterpart (liquid's
 * firpfbch family is the same structure); the definition is this library's
 * own.  For the concatenated input x[t] (zeros before the first sample and
 * after reset), a real prototype h of L taps, M channels and decimation D:
 *   y[k][n] = scale sum_{j<L} h[j] x[nD - j] exp(-2 pi i k (nD - j) / M)
 * i.e. mix down by k / M cycles per sample, filter with h, keep every D-th
 * sample starting at t = 0.  Channel k is centred at k / M; k >= M / 2 are the
 * negative frequencies (FFT order).  Output n is emitted by the call that
 * delivers x[nD]: with T samples seen before a call and skip = (-T) mod D, a
 * call of n samples returns n > skip ? ceil((n - skip) / D) : 0 columns; calls
 * of any length, 0 included, are allowed.
 *   M: a power of two, 4 <= M <= 256;  D = M (critically sampled) or M / 2 (2x
 *   oversampled);  at most 17 taps per branch (L <= 17 M; m <= 8).
 * ldsp_chan_create designs h = firdes_kaiser(2 M m + 1, fc, as, 0) (fc <= 0:
 * 0.5 / M) and sets scale = 1 / sum(h) (unit gain at a channel's centre);
 * ldsp_chan_create_taps takes h as given with scale = 1.  A non-power-of-two
 * M, M < 4, another D, m = 0, L = 0, as <= 0 and fc >= 0.5 are LDSP_EINVAL; a
 * power-of-two M above 256 and more than 17 taps per branch are LDSP_EUNSUP.
 * ldsp_chan_execute writes row k to y + k * ld (ld in samples); it sets *ncols
 * and, when ld < *ncols, returns LDSP_ERANGE without consuming the input.
 * Argument errors are decided on the host before any device work.
 * ---------------------------------------------------------------------- */
typedef struct ldsp_chan_s *ldsp_chan_t;
int ldsp_chan_create(unsigned int M, unsigned int D, unsigned int m, float fc, float as, ldsp_chan_t *q);
int ldsp_chan_create_taps(unsigned int M, unsigned int D, const float *h, unsigned int L, ldsp_chan_t *q);
int ldsp_chan_destroy(ldsp_chan_t q);
int ldsp_chan_reset(ldsp_chan_t q);
/* Any pointer may be NULL.  skip: input samples before the next call's first output. */
int ldsp_chan_get_info(ldsp_chan_t q, unsigned int *M, unsigned int *D, unsigned int *L, unsigned int *skip);
int ldsp_chan_get_taps(ldsp_chan_t q, float *h);                 /* L floats */
int ldsp_chan_get_scale(ldsp_chan_t q, float *s);
int ldsp_chan_set_scale(ldsp_chan_t q, float s);
int ldsp_chan_num_outputs(ldsp_chan_t q, size_t n, size_t *ncols);
int ldsp_chan_execute(ldsp_chan_t q, const void *x, size_t n, void *y, size_t ld, size_t *ncols, int mem,
                      void *stream);
/* ldsp_bytes_to_iq fused into the bank's loads: x holds n native int16 (I, Q)
 * pairs (4 n bytes, 4-byte aligned; n counts pairs), each converted to
 * (float)v / 32767.0f as bytes_to_iq does.  Everything else is
 * ldsp_chan_execute's: the same checks, *ncols and rows, the bits of
 * ldsp_bytes_to_iq followed by ldsp_chan_execute, and the same state after the
 * call (the history is kept as complex64), so the calls of one stream may be of
 * either kind.  A host input stages 4 n bytes. */
int ldsp_chan_execute_iq16(ldsp_chan_t q, const void *x, size_t n, void *y, size_t ld, size_t *ncols, int mem,
                           void *stream);
/* Test hook: output frames (columns) per workgroup of the (M, D) kernel. */
int ldsp_debug_chan_tile(unsigned int M, unsigned int D, size_t *frames);

/* ------------------------------------------------------------------------
 * Synthesizer: a polyphase synthesis filter bank, M channel rows to one
 * dense complex64 stream in one pass; the Channelizer's counterpart.  The
 * definition is this library's own.  Column n and output sample t are absolute
 * indices since creation or reset (zeros before column 0); g is a real
 * prototype of L taps, M the channel count and D the interpolation:
 *   z[t] = scale sum_{k<M} sum_{n : 0 <= t - nD < L} g[t - nD] y[k][n] exp(+2 pi i k t / M)
 * i.e. zero-stuff every row by D, filter with g, mix row k up to k / M cycles
 * per sample with the phase tied to absolute t, and sum the rows.  A call of
 * ncols columns returns exactly ncols * D samples (ncols = 0 is allowed); a
 * stream of columns may be cut into calls anywhere without changing a bit.
 *   M: a power of two, 4 <= M <= 256;  D = M (critically sampled) or M / 2 (2x
 *   oversampled);  at most 17 taps per branch (L <= 17 M; m <= 8).
 * ldsp_synth_create designs g = firdes_kaiser(2 M m + 1, fc, as, 0) (fc <= 0:
 * 1 / M at D = M / 2, 0.5 / M at D = M) and sets scale = D / sum(g);
 * ldsp_synth_create_taps takes g as given with scale = 1.  With the defaults
 * at D = M / 2, ldsp_chan_create(M, M / 2, m, 0, as) followed by
 * ldsp_synth_create(M, M / 2, m, 0, as) reproduces the input delayed by
 * L - 1 = 2 M m samples, to the prototype's stop-band level 10^(-as / 20).
 * The error codes are the Channelizer's: a non-power-of-two M, M < 4, another
 * D, m = 0, L = 0, as <= 0 and fc >= 0.5 are LDSP_EINVAL; a power-of-two M
 * above 256 and more than 17 taps per branch are LDSP_EUNSUP.
 * ldsp_synth_execute reads row k at y + k * ld (ld in samples; ld < ncols is
 * LDSP_EINVAL) and writes ncols * D samples to z; it sets *n and, when
 * cap < *n, returns LDSP_ERANGE without consuming the input.  Argument errors
 * are decided on the host before any device work.
 * ---------------------------------------------------------------------- */
typedef struct ldsp_synth_s *ldsp_synth_t;
int ldsp_synth_create(unsigned int M, unsigned int D, unsigned int m, float fc, float as, ldsp_synth_t *q);
int ldsp_synth_create_taps(unsigned int M, unsigned int D, const float *g, unsigned int L, ldsp_synth_t *q);
int ldsp_synth_destroy(ldsp_synth_t q);
int ldsp_synth_reset(ldsp_synth_t q);
int ldsp_synth_get_info(ldsp_synth_t q, unsigned int *M, unsigned int *D, unsigned int *L);   /* any may be NULL */
int ldsp_synth_get_taps(ldsp_synth_t q, float *g);               /* L floats */
int ldsp_synth_get_scale(ldsp_synth_t q, float *s);
int ldsp_synth_set_scale(ldsp_synth_t q, float s);
int ldsp_synth_num_outputs(ldsp_synth_t q, size_t ncols, size_t *n);
int ldsp_synth_execute(ldsp_synth_t q, const void *y, size_t ld, size_t ncols, void *z, size_t cap, size_t *n,
                       int mem, void *stream);
/* Test hook: input columns per workgroup of the (M, D) kernel. */
int ldsp_debug_synth_tile(unsigned int M, unsigned int D, size_t *cols);

/* ------------------------------------------------------------------------
 * Downconverter: a bank of C independently tuned decimating filters ("tune,
 * low-pass, decimate") over one wideband complex64 stream, read once.
 * liquid's counterpart is nco_crcf + firdecim_crcf; the definition is this
 * library's own.  For the concatenated input x[t] (t counted from 0 since
 * creation or reset, zeros before it), a real prototype h of L taps, a
 * decimation D and tuners c < C with 32-bit frequency words w_c:
 *   phase(c, t) = (t w_c) mod 2^32                       (integers, exact for any t)
 *   y[c][n]     = scale sum_{j<L} h[j] x[nD - j] exp(-2 pi i phase(c, nD - j) / 2^32)
 * w_c = rint(f_c 2^32) mod 2^32 for a frequency f_c in cycles per sample (a
 * finite double, |f_c| <= 1; the product is exact, ties go to even); the
 * tuner's true frequency is w_c / 2^32.  The sum is evaluated as
 *   g_c[j]   = h[j] exp(+2 pi i ((j w_c) mod 2^32) / 2^32)        (double, rounded once)
 *   y[c][n]  = scale rot_c(n) sum_j g_c[j] x[nD - j]
 *   rot_c(n) = exp(-2 pi i (((nD) mod 2^32) w_c mod 2^32) / 2^32)
 * which is the same sum, the phase being additive modulo 2^32.  The column
 * schedule is the Channelizer's: output n is emitted by the call that delivers
 * x[nD]; with T samples seen before a call and skip = (-T) mod D, a call of n
 * samples returns n > skip ? ceil((n - skip) / D) : 0 columns; calls of any
 * length, 0 included, are allowed.  A row's bits depend neither on how the
 * stream is cut into calls nor on the other tuners, their number or order.
 *   2 <= D <= 256, any integer;  1 <= C <= 64;  1 <= L <= 17 D;  1 <= m <= 8.
 * ldsp_ddc_create designs h = firdes_kaiser(2 D m + 1, fc, as, 0) (fc <= 0:
 * 0.5 / D) and sets scale = 1 / sum(h); ldsp_ddc_create_taps takes h as given
 * with scale = 1.  D = 0, C = 0, L = 0, m = 0, as <= 0, fc >= 0.5, a NULL f and
 * an f_c that is not finite or above 1 in magnitude are LDSP_EINVAL; D = 1
 * (ldsp_nco_mix_firfilt serves it), D > 256, C > 64, L > 17 D and m > 8 are
 * LDSP_EUNSUP.  ldsp_ddc_set_frequencies retunes (C may change): the history
 * holds raw input, so the following columns are those of a bank created with
 * the new list and fed the same stream in the same cuts.  ldsp_ddc_execute
 * writes row c to y + c * ld (ld in samples); it sets *ncols and, when
 * ld < *ncols, returns LDSP_ERANGE without consuming the input.  Argument
 * errors are decided on the host before any device work.
 * Not built: D = 1, real input, per-tuner prototypes or decimations, a
 * fast-convolution (FFT) form.
 * ---------------------------------------------------------------------- */
typedef struct ldsp_ddc_s *ldsp_ddc_t;
int ldsp_ddc_create(const double *f, unsigned int C, unsigned int D, unsigned int m, float fc, float as,
                    ldsp_ddc_t *q);
int ldsp_ddc_create_taps(const double *f, unsigned int C, unsigned int D, const float *h, unsigned int L,
                         ldsp_ddc_t *q);
int ldsp_ddc_destroy(ldsp_ddc_t q);
int ldsp_ddc_reset(ldsp_ddc_t q);
int ldsp_ddc_set_frequencies(ldsp_ddc_t q, const double *f, unsigned int C);   /* C may change, 1..64 */
int ldsp_ddc_get_words(ldsp_ddc_t q, uint32_t *w);                             /* C words */
/* Any pointer may be NULL.  skip: input samples before the next call's first output. */
int ldsp_ddc_get_info(ldsp_ddc_t q, unsigned int *C, unsigned int *D, unsigned int *L, unsigned int *skip);
int ldsp_ddc_get_taps(ldsp_ddc_t q, float *h);                   /* L floats */
int ldsp_ddc_get_scale(ldsp_ddc_t q, float *s);
int ldsp_ddc_set_scale(ldsp_ddc_t q, float s);
int ldsp_ddc_num_outputs(ldsp_ddc_t q, size_t n, size_t *ncols);
int ldsp_ddc_execute(ldsp_ddc_t q, const void *x, size_t n, void *y, size_t ld, size_t *ncols, int mem,
                     void *stream);
/* ldsp_bytes_to_iq fused into the bank's loads, as ldsp_chan_execute_iq16: x
 * holds n native int16 (I, Q) pairs (4 n bytes, 4-byte aligned); the checks,
 * *ncols, the rows' bits and the state after the call are those of
 * ldsp_bytes_to_iq followed by ldsp_ddc_execute (the history holds the
 * converted samples, so retuning and mixed call kinds work as before). */
int ldsp_ddc_execute_iq16(ldsp_ddc_t q, const void *x, size_t n, void *y, size_t ld, size_t *ncols, int mem,
                          void *stream);
/* Test hook: output columns per workgroup of the (D, L) kernel. */
int ldsp_debug_ddc_tile(unsigned int D, unsigned int L, size_t *frames);
/* Test hook: reset, then place the stream at sample T (zero history), to reach
 * the phase arithmetic near T = 2^32 without streaming that far. */
int ldsp_debug_ddc_seek(ldsp_ddc_t q, uint64_t T);

/* ------------------------------------------------------------------------
 * FMBank: for every row of a complex64 [C][K] block (a Channelizer or
 * Downconverter output, read in place), FreqDem's discriminator followed by a
 * real decimating FIR, in one pass; the full-rate discriminator output stays
 * on the chip.  liquid's counterpart is freqdem + firdecim_rrrf per row; the
 * definition is this library's own.  For row c of the concatenated input
 * x[c][t] (t counted from 0 since creation or reset; the sample before t = 0
 * is 0, as after freqdem_reset), ref = (float)(1 / (2 pi kf)) computed as in
 * ldsp_freqdem_create, a real prototype h of L taps and a decimation D:
 *   d[c][t] = lm_atan2f(im, re) * ref,   (re, im) = conj(x[c][t-1]) * x[c][t]
 *   y[c][n] = scale sum_{j<L} h[j] d[c][nD - j]            (d = 0 before t = 0)
 * d[c][t] is computed operation for operation as ldsp_freqdem_demodulate
 * computes it.  The column schedule is the Channelizer's: output n is emitted
 * by the call that delivers sample nD of every row; with T samples per row seen
 * before a call and skip = (-T) mod D, a call of K samples per row returns
 * K > skip ? ceil((K - skip) / D) : 0 columns; calls of any K, 0 included, are
 * allowed.  A row's bits depend neither on how the stream is cut into calls nor
 * on the other rows, their number or order.
 *   1 <= C <= 256, fixed at creation;  kf > 0;  1 <= D <= 64;  1 <= L <= 17 D;
 *   1 <= m <= 8.
 * ldsp_fmbank_create designs h = firdes_kaiser(2 D m + 1, fc, as, 0) (fc <= 0:
 * 0.5 / D) and sets scale = 1 / sum(h); with D = 1 it designs nothing and the
 * object is the discriminator alone: y = d with no filter arithmetic, every row
 * ldsp_freqdem_demodulate's bits, L reported as 0, scale 1 and not settable.
 * ldsp_fmbank_create_taps takes h as given with scale = 1 (D = 1 allowed: a
 * full-rate filter).  C, D or kf out of range, L = 0, m = 0, as <= 0 and
 * fc >= 0.5 are LDSP_EINVAL; L > 17 D and m > 8 are LDSP_EUNSUP.
 * ldsp_fmbank_execute reads row c at x + c * ldx and writes float32 row c to
 * y + c * ldy (both in samples, ldx >= K); it sets *ncols and, when
 * ldy < *ncols, returns LDSP_ERANGE without consuming the input.  Argument
 * errors are decided on the host before any device work.
 * De-emphasis and rate conversion over the rows it writes: AudioBank, below;
 * a squelch over the rows it reads: SquelchBank, below.
 * Not built: a per-row kf.
 * ---------------------------------------------------------------------- */
typedef struct ldsp_fmbank_s *ldsp_fmbank_t;
int ldsp_fmbank_create(unsigned int C, float kf, unsigned int D, unsigned int m, float fc, float as, ldsp_fmbank_t *q);
int ldsp_fmbank_create_taps(unsigned int C, float kf, unsigned int D, const float *h, unsigned int L,
                            ldsp_fmbank_t *q);
int ldsp_fmbank_destroy(ldsp_fmbank_t q);
int ldsp_fmbank_reset(ldsp_fmbank_t q);
/* Any pointer may be NULL.  skip: input samples per row before the next call's first output. */
int ldsp_fmbank_get_info(ldsp_fmbank_t q, unsigned int *C, unsigned int *D, unsigned int *L, unsigned int *skip);
int ldsp_fmbank_get_taps(ldsp_fmbank_t q, float *h);             /* L floats */
int ldsp_fmbank_get_scale(ldsp_fmbank_t q, float *s);
int ldsp_fmbank_set_scale(ldsp_fmbank_t q, float s);             /* LDSP_EINVAL for the discriminator alone */
int ldsp_fmbank_num_outputs(ldsp_fmbank_t q, size_t K, size_t *ncols);
int ldsp_fmbank_execute(ldsp_fmbank_t q, const void *x, size_t ldx, size_t K, void *y, size_t ldy, size_t *ncols,
                        int mem, void *stream);
/* Test hook: output columns per workgroup of the (D, L) kernel (L = 0: the discriminator alone). */
int ldsp_debug_fmbank_tile(unsigned int D, unsigned int L, size_t *frames);

/* ------------------------------------------------------------------------
 * AudioBank: for every row of a float32 [C][K] block (an FMBank output, read in
 * place), an optional one-pole de-emphasis at the input rate followed by
 * liquid's arbitrary-rate polyphase resampler and an optional 16-bit PCM store,
 * in one pass; the de-emphasised signal stays on the chip.  liquid's
 * counterpart is iirfilt_rrrf (one pole) + resamp_rrrf per row (the reference's
 * FM receiver, src/demod.hpp:19-31, 75-82).  For row c of the concatenated
 * input u[c][t] (t counted from 0 since creation or reset, u = 0 before that):
 *   a  = (float) exp(-1 / (tau * (double)sample_rate)),   b0 = (float)(1 - (double)a)
 *   e[c][t] = b0 sum_{j>=0} a^j u[c][t-j]         (de-emphasis off: e = u, no arithmetic)
 *   y[c][k] = sum_{n<2m} h_{b_k}[n] e[c][j_k - n]
 *   z = y * scale;   float32 out = z;
 *   pcm16 out = (int16) clamp(rintf(z * 32767.0f), -32768, 32767)
 * The prototype, the rounding of npfb to a power of two, step = round(2^24 /
 * rate), the fixed-point phase schedule (j_k, b_k) and the dot product's order
 * are ldsp_resamp's (kind 0, resamp_rrrf): without de-emphasis and at scale 1
 * every row carries ldsp_resamp_execute's bits, and *nout is its count call by
 * call, the same for every row.  At tau = 75e-6 the coefficients a and b0 are
 * DeemphasisFilter's.  With de-emphasis every row is within 1e-6 of the float64
 * evaluation of the lines above (max-norm, relative to the row's maximum); the
 * recursion's state is kept in float64 (liquid's float32 state misses that gate
 * on a constant row).  A row's bits depend neither on how the stream is cut into
 * calls, nor on the other rows, their number or order, nor on the row strides.
 *   1 <= C <= 256, fixed at creation;  1/32 <= rate <= 4;  1 <= m <= 32;
 *   npfb (rounded) * 2m <= 8192;  tau * sample_rate <= 32 input samples.
 * ldsp_audiobank_create: sample_rate <= 0 means no de-emphasis (tau is then not
 * looked at).  C out of range, rate <= 0, m = 0, fc outside (0, 0.5), as <= 0,
 * npfb = 0, and tau <= 0 with de-emphasis are LDSP_EINVAL; a rate outside
 * [1/32, 4], m > 32, more than 8192 branch taps and tau * sample_rate > 32 are
 * LDSP_EUNSUP.
 * ldsp_audiobank_execute reads row c at x + c * ldx and writes row c (float32,
 * or int16 with pcm16) to y + c * ldy, both in samples (ldx >= K); it sets *nout
 * and, when ldy < *nout, returns LDSP_ERANGE without consuming the input.
 * K = 0 and calls too short for an output are allowed; they carry state only.
 * Argument errors are decided on the host before any device work.
 * Not built: a mid-stream rate setter, complex rows, per-row rates or time
 * constants, de-emphasis after the resampler.
 * ---------------------------------------------------------------------- */
typedef struct ldsp_audiobank_s *ldsp_audiobank_t;
int ldsp_audiobank_create(unsigned int C, float rate, unsigned int m, float fc, float as, unsigned int npfb,
                          float sample_rate, double tau, int pcm16, ldsp_audiobank_t *q);
int ldsp_audiobank_destroy(ldsp_audiobank_t q);
int ldsp_audiobank_reset(ldsp_audiobank_t q);
/* Any pointer may be NULL.  npfb: after the rounding; phase: the schedule's, as ldsp_resamp_get_info's. */
int ldsp_audiobank_get_info(ldsp_audiobank_t q, unsigned int *C, unsigned int *npfb, uint32_t *step, uint32_t *phase,
                            unsigned int *sub_len);
/* As ldsp_resamp_get_taps: the prototype of 2 m npfb + 1 taps; h may be NULL to ask for *n. */
int ldsp_audiobank_get_taps(ldsp_audiobank_t q, float *h, unsigned int cap, unsigned int *n);
/* Any pointer may be NULL.  Without de-emphasis: b0 = 1, a = 0, sample_rate = 0, tau = 0. */
int ldsp_audiobank_get_coefs(ldsp_audiobank_t q, float *b0, float *a, float *sample_rate, double *tau);
int ldsp_audiobank_get_scale(ldsp_audiobank_t q, float *s);
int ldsp_audiobank_set_scale(ldsp_audiobank_t q, float s);
int ldsp_audiobank_num_outputs(ldsp_audiobank_t q, size_t K, size_t *nout);
int ldsp_audiobank_execute(ldsp_audiobank_t q, const void *x, size_t ldx, size_t K, void *y, size_t ldy, size_t *nout,
                           int mem, void *stream);
/* Test hook: outputs per workgroup of the kernel this object launches. */
int ldsp_debug_audiobank_tile(ldsp_audiobank_t q, size_t *outputs);

/* ------------------------------------------------------------------------
 * SquelchBank: for every row of a complex64 [C][K] block (a Channelizer or
 * Downconverter output, read in place), the row's smoothed power per block of
 * B samples, liquid's squelch state per block and, optionally, the rows
 * themselves with the closed blocks zeroed.  liquid's counterpart is the
 * squelch half of agc_crcf, evaluated per block of samples instead of per
 * sample and with no gain loop; the definition is this library's own.  For row
 * c of the concatenated input x[c][t] (t counted from 0 since creation or
 * reset), B = block, alpha = bandwidth (a double) and thr[c] the float32
 * rounding of 10^(threshold_dB[c] / 10) computed in double:
 *   p[c][b] = (1/B) sum_{i<B} |x[c][bB + i]|^2                     block power
 *   s[c][b] = s[c][b-1] + alpha (p[c][b] - s[c][b-1]),  s[c][-1] = 0   (float64)
 *   level[c][b] = (float) s[c][b]                        float32, linear power
 *   hi = level[c][b] > thr[c]              in float32, on the value stored
 *   mode[c][b] = liquid's agc squelch step from mode[c][b-1] with hi:
 *     ENABLED(1):  hi ? RISE : ENABLED          RISE(2): hi ? SIGNALHI : FALL
 *     SIGNALHI(3): hi ? SIGNALHI : FALL
 *     FALL(4):     hi ? SIGNALHI : SIGNALLO, timer = timeout
 *     SIGNALLO(5): --timer == 0 ? TIMEOUT : (hi ? SIGNALHI : SIGNALLO)
 *     TIMEOUT(6):  ENABLED                      initial mode ENABLED, timer 0
 *   status[c][b] = mode[c][b]                           uint8, liquid's codes
 *   open = status in {RISE, SIGNALHI, FALL, SIGNALLO}
 *   y[c][bB + i] = open ? x[c][bB + i] (the same bits) : +0.0
 * The step is agc_squelch_update_mode, once per block: timeout counts blocks.
 * The gate rule is this object's own: the reference's AGC wrapper zeroes
 * SIGNALLO and passes TIMEOUT, which makes the time-out useless as a hang time;
 * here SIGNALLO stays open and TIMEOUT is closed.  status is an exact function
 * of the level output.
 * Block b is emitted by the call that delivers its last sample: with T samples
 * per row seen before a call, a call of K samples returns
 * (T + K) / B - T / B blocks (integer division); K = 0 and calls too short for
 * a block are allowed and carry state only.  The fill = (T + K) mod B samples of
 * the unfinished block are carried to the next call, so the gated output of a
 * call, complex64 [C][nblocks B], starts with the carried samples: the rows stay
 * one contiguous stream, delayed to block boundaries.  A row's bits (level,
 * status, gated samples) depend neither on how the stream is cut into calls,
 * nor on the other rows, their number or order, nor on the row strides.
 *   1 <= C <= 256, fixed at creation;  16 <= B <= 4096 (any integer);
 *   0 < alpha <= 1;  timeout >= 1;  thresholds finite.
 * Anything else (a NaN among them) is LDSP_EINVAL.
 * ldsp_sqbank_create sets every row's threshold to threshold_dB;
 * ldsp_sqbank_set_thresholds takes n = 1 (every row) or n = C values, takes
 * effect at the next block and touches no state; ldsp_sqbank_reset restores the
 * initial state and keeps the thresholds.
 * ldsp_sqbank_execute reads row c at x + c * ldx (samples, ldx >= K) and writes
 * row c of status to status + c * lds (bytes), of level to level + c * ldl
 * (floats) and, where y is not NULL, of the gated samples to y + c * ldy
 * (samples); with y == NULL it only measures.  It sets *nblocks and, when lds or
 * ldl < *nblocks or ldy < *nblocks B, returns LDSP_ERANGE without consuming the
 * input.  Argument errors are decided on the host before any device work.
 * ldsp_sqbank_get_state copies out, per row, the mode, the timer and s after
 * the last call; it waits for that call.
 * Not built: a per-sample squelch, a per-row block or bandwidth, callbacks on
 * rise, squelch inside ldsp_agc_execute_many, skipping closed rows inside
 * FMBank / AudioBank, a noise-floor-tracking automatic threshold, in-place
 * gating.
 * ---------------------------------------------------------------------- */
typedef struct ldsp_sqbank_s *ldsp_sqbank_t;
int ldsp_sqbank_create(unsigned int C, unsigned int B, double alpha, double threshold_dB, unsigned int timeout,
                       ldsp_sqbank_t *q);
int ldsp_sqbank_destroy(ldsp_sqbank_t q);
int ldsp_sqbank_reset(ldsp_sqbank_t q);
int ldsp_sqbank_set_thresholds(ldsp_sqbank_t q, const double *dB, unsigned int n);  /* n = 1 or C */
/* Either pointer may be NULL; C values each: dB as set, lin as the kernel compares. */
int ldsp_sqbank_get_thresholds(ldsp_sqbank_t q, double *dB, float *lin);
/* Any pointer may be NULL.  fill: samples per row carried to the next call. */
int ldsp_sqbank_get_info(ldsp_sqbank_t q, unsigned int *C, unsigned int *B, double *alpha, unsigned int *timeout,
                         unsigned int *fill);
int ldsp_sqbank_num_outputs(ldsp_sqbank_t q, size_t K, size_t *nblocks);
int ldsp_sqbank_execute(ldsp_sqbank_t q, const void *x, size_t ldx, size_t K, uint8_t *status, size_t lds, float *level,
                        size_t ldl, void *y, size_t ldy, size_t *nblocks, int mem, void *stream);
/* Any pointer may be NULL; C values each. */
int ldsp_sqbank_get_state(ldsp_sqbank_t q, int *mode, unsigned int *timer, double *s);
/* Test hook: blocks per workgroup of the power kernel. */
int ldsp_debug_sqbank_tile(unsigned int B, size_t *blocks);

/* ------------------------------------------------------------------------
 * StereoBank: for every row of a float32 [C][K] block of FM multiplex (MPX)
 * samples (the output of an FMBank(C, kf, 1), read in place), a feed-forward FM
 * stereo decoder: the mono sum, the 38 kHz difference and the 19 kHz pilot by
 * three decimating FIRs over one read of the row, and left and right from
 * them, in one launch for all rows.  The reference's FMStereo (one stream, a
 * per-sample pilot PLL) is a different decoder and stays as it is; the
 * definition here is this library's own.  For row c of the concatenated input
 * u[c][t] (t counted from 0 since creation or reset, u = 0 before t = 0), the
 * 32-bit pilot word w = rint(pilot 2^32) mod 2^32 (pilot in cycles per sample,
 * 19 kHz / fs; the product is exact, ties go to even), a decimation D, two real
 * prototypes of the same length L, h for the audio and g for the pilot, and a
 * pilot threshold thr:
 *   s[c][n] = sum_{j<L} h[j] u[c][nD-j]
 *   z[c][n] = sum_{j<L} h[j] u[c][nD-j] exp(-2 pi i (((nD-j) * 2w) mod 2^32) / 2^32)
 *   P[c][n] = sum_{j<L} g[j] u[c][nD-j] exp(-2 pi i (((nD-j) *  w) mod 2^32) / 2^32)
 *   m       = |P|^2                         (float32, on the value the kernel holds)
 *   S       = m > thr^2 ? 2 Im(z conj(P)^2) / m : 0          (thr^2 = thr * thr in float32)
 *   left[c][n] = s + S ,  right[c][n] = s - S
 * For the standard multiplex 0.45 (l + r) + 0.45 (l - r) sin 2 theta +
 * a_p sin theta this gives left = 0.9 l and right = 0.9 r delayed by (L - 1) / 2
 * input samples: conj(P)^2 / |P|^2 carries the pilot's doubled phase, whatever
 * its offset from the nominal frequency is inside g's pass band, so nothing is
 * tracked from column to column and a row has no serial state but its last
 * L - 1 raw samples.  Below the threshold the row is mono: left = right = s,
 * the same bits.
 * The sums are evaluated with the complex taps
 *   gz[j] = h[j] exp(+2 pi i ((j 2w) mod 2^32) / 2^32)          (double, rounded once)
 *   gp[j] = g[j] exp(+2 pi i ((j  w) mod 2^32) / 2^32)
 *   z' = sum_j gz[j] u[c][nD-j],   P' = sum_j gp[j] u[c][nD-j]
 * The phase is additive modulo 2^32, so z = rz z' and P = rp P' with
 * rp = exp(-2 pi i ((nD w) mod 2^32) / 2^32) and rz likewise with 2w; and
 * (nD 2w) mod 2^32 = 2 ((nD w) mod 2^32) mod 2^32, so rz = rp^2 exactly,
 * z conj(P)^2 = z' conj(P')^2 and |P| = |P'|: neither m nor S depends on the
 * per-output rotations, and they are not applied.  No step depends on the
 * stream position beyond skip, so the result is exact for any stream length.
 * Every row of left and right is within 1e-6 of the float64 evaluation of the
 * definition (max-norm, relative to the row's maximum) for a pilot of
 * amplitude 0.1; a weaker pilot divides the same absolute error by a smaller m.
 * The column schedule is the Channelizer's and the FMBank's: output n is
 * emitted by the call that delivers sample nD of every row; with T samples per
 * row seen before a call and skip = (-T) mod D, a call of K samples per row
 * returns K > skip ? ceil((K - skip) / D) : 0 columns; calls of any K, 0
 * included, are allowed.  A row's bits depend neither on how the stream is cut
 * into calls, nor on the other rows, their number or order, nor on the row
 * strides.
 *   1 <= C <= 128, fixed at creation (the 2 C output rows fit an AudioBank);
 *   1 <= D <= 32;  1 <= L <= 1025;  0 < pilot < 0.25;  thr >= 0;  as > 0.
 * ldsp_stbank_create designs, with L = 0 standing for 2 ceil(8.5 / pilot) + 1,
 *   h = firdes_kaiser(L, (float)((17/19) pilot), as, 0),
 *   g = firdes_kaiser(L, (float)(( 2/19) pilot), as, 0),
 * each tap then divided in double by the double sum of the float32 design and
 * rounded once (unit DC gain).  ldsp_stbank_create_taps takes h and g as given;
 * they must have the same length.  A value out of range (a NaN among them), a
 * NULL pointer and prototypes of unequal length are LDSP_EINVAL; a default L
 * above 1025 (pilot below about 0.0166) is LDSP_EUNSUP.
 * ldsp_stbank_set_threshold takes effect at the next call and touches no state.
 * ldsp_stbank_execute reads row c at x + c * ldx and writes left of row c to
 * y + (2 c) * ldy and right to y + (2 c + 1) * ldy (all in samples, ldx >= K):
 * the output is a [2 C][ncols] image an AudioBank(2 C, ...) reads in place.  It
 * sets *ncols and, when ldy < *ncols, returns LDSP_ERANGE without consuming the
 * input.  Argument errors are decided on the host before any device work.
 * ldsp_stbank_get_pilot_level copies out, per row, sqrtf(m) of the last column
 * emitted (0 before any); it waits for the last call.
 * Not built: smoothing of P across columns, a stereo blend, RDS, a per-row
 * pilot or threshold, any change of the reference-parity FMStereo.
 * ---------------------------------------------------------------------- */
typedef struct ldsp_stbank_s *ldsp_stbank_t;
/* L = 0: the default length. */
int ldsp_stbank_create(unsigned int C, double pilot, unsigned int D, unsigned int L, float as, float threshold,
                       ldsp_stbank_t *q);
int ldsp_stbank_create_taps(unsigned int C, double pilot, unsigned int D, const float *h, unsigned int L,
                            const float *g, unsigned int Lg, float threshold, ldsp_stbank_t *q);
int ldsp_stbank_destroy(ldsp_stbank_t q);
int ldsp_stbank_reset(ldsp_stbank_t q);
/* Any pointer may be NULL.  skip: input samples per row before the next call's first output; w: the pilot word. */
int ldsp_stbank_get_info(ldsp_stbank_t q, unsigned int *C, unsigned int *D, unsigned int *L, unsigned int *skip,
                         uint32_t *w);
int ldsp_stbank_get_taps(ldsp_stbank_t q, float *h, float *g);   /* L floats each; either may be NULL */
int ldsp_stbank_get_threshold(ldsp_stbank_t q, float *thr);
int ldsp_stbank_set_threshold(ldsp_stbank_t q, float thr);
int ldsp_stbank_num_outputs(ldsp_stbank_t q, size_t K, size_t *ncols);
int ldsp_stbank_execute(ldsp_stbank_t q, const void *x, size_t ldx, size_t K, void *y, size_t ldy, size_t *ncols,
                        int mem, void *stream);
int ldsp_stbank_get_pilot_level(ldsp_stbank_t q, float *level);  /* C floats */
/* Test hook: output columns per workgroup of the (D, L) kernel. */
int ldsp_debug_stbank_tile(unsigned int D, unsigned int L, size_t *frames);

/* ------------------------------------------------------------------------
 * AMBank: a feed-forward coherent AM demodulator over the rows of a bank.  Every
 * row of a complex64 [C][K] block (a Channelizer, Downconverter or SquelchBank
 * output) goes to one row of float32 audio, in one launch for all rows.  No
 * reference counterpart: liquid's ampmodem (AmpModem, BroadcastAM) tracks the
 * carrier with a per-sample PLL behind an AGC, one stream per object; this
 * decoder has no loop to lock, and the definition is this library's own.  With
 * a decimation D, an audio prototype h, a carrier prototype g of the same
 * length L (real, float32) and a threshold thr, for every row c, with zeros
 * before the stream's start:
 *   d[j]     = (float)((double)h[j] - (double)g[j])                (rounded once)
 *   B[c][n]  = sum_{j<L} d[j] x[c][nD-j]      (complex: the audio band, the carrier taken out)
 *   Cr[c][n] = sum_{j<L} g[j] x[c][nD-j]      (complex: the carrier)
 *   m        = |Cr|^2                         (float32, on the value the kernel holds)
 *   y[c][n]  = m > thr^2 ? Re(B conj(Cr)) / m : 0                  (thr^2 = thr * thr in float32)
 * For x = A (1 + a(t)) exp(i (2 pi f0 t + phi)) with f0 inside g's pass band, Cr
 * is the carrier and B is A a(t) exp(i theta), so y = a(t) delayed by
 * (L - 1) / 2 input samples: full scale +-1 is 100 % modulation whatever A, phi
 * and f0 are, nothing is tracked from column to column, there is no AGC, and a
 * row has no serial state but its last L - 1 raw samples.  B is formed with d
 * and not as (h * x) - Cr, so the carrier never has to cancel in float32.  A row
 * of zeros (a block a SquelchBank closed) gives m = 0 and y = +0, never 0 / 0,
 * at any threshold.  m, the product and the division are single float32
 * operations (the two sums of two products each one fused multiply-add).
 * Every row of y is within 1e-6 of the float64 evaluation of the definition
 * (max-norm, absolute: against the scale of the carrier, y = 1 being 100 %)
 * wherever |B| <= |Cr|, which is every column of a row with a carrier once its
 * window lies inside the stream.  Where |B| > |Cr| (the first columns of a
 * stream, whose carrier estimate is a few edge taps, and rows without a carrier
 * at a low threshold) y is unbounded and the error is within 1e-6 of
 * SB / |Cr| + |B| SC / |Cr|^2, SB = sum |d[j] x|, SC = sum |g[j] x|.
 * The column schedule is the Channelizer's and the FMBank's: output n is
 * emitted by the call that delivers sample nD of every row; with T samples per
 * row seen before a call and skip = (-T) mod D, a call of K samples per row
 * returns K > skip ? ceil((K - skip) / D) : 0 columns; calls of any K, 0
 * included, are allowed.  A row's bits depend neither on how the stream is cut
 * into calls, nor on the other rows, their number or order, nor on the row
 * strides.
 *   1 <= C <= 256, fixed at creation;  1 <= D <= 32;  1 <= L <= 1025;
 *   0 < carrier < audio <= 0.5 (cycles per row sample);  thr >= 0;  as > 0.
 * ldsp_ambank_create designs, with audio = 0 standing for 0.5 / D (0.45 when
 * D = 1) and L = 0 for 2 ceil(2 / carrier) + 1 (1001 at carrier = 0.004; a 60 dB
 * Kaiser's transition is then about 0.9 carrier and g stops from about
 * 1.45 carrier),
 *   h = firdes_kaiser(L, (float)audio, as, 0),
 *   g = firdes_kaiser(L, (float)carrier, as, 0),
 * each tap then divided in double by the double sum of the float32 design and
 * rounded once (unit DC gain).  ldsp_ambank_create_taps takes h and g as given;
 * they must have the same length.  A value out of range (a NaN among them), a
 * NULL pointer and prototypes of unequal length are LDSP_EINVAL; a default L
 * above 1025 (carrier below 2 / 512) is LDSP_EUNSUP.
 * ldsp_ambank_set_threshold takes effect at the next call and touches no state.
 * ldsp_ambank_execute reads row c at x + c * ldx and writes row c at
 * y + c * ldy (all in samples, ldx >= K): the output is a [C][ncols] image an
 * AudioBank(C, ...) reads in place.  It sets *ncols and, when ldy < *ncols,
 * returns LDSP_ERANGE without consuming the input.  Argument errors are decided
 * on the host before any device work.
 * ldsp_ambank_get_carrier_level copies out, per row, sqrtf(m) of the last
 * column emitted (0 before any); it waits for the last call.
 * Not built: a per-row carrier offset or search, suppressed-carrier (DSB-SC)
 * rows (single-sideband rows are the SSBBank's), a two-stage (decimate first)
 * carrier estimate, envelope output, skipping closed rows, any change of
 * AmpModem / BroadcastAM / execute_many.
 * ---------------------------------------------------------------------- */
typedef struct ldsp_ambank_s *ldsp_ambank_t;
/* audio = 0: the default cut-off;  L = 0: the default length. */
int ldsp_ambank_create(unsigned int C, unsigned int D, double audio, double carrier, unsigned int L, float as,
                       float threshold, ldsp_ambank_t *q);
int ldsp_ambank_create_taps(unsigned int C, unsigned int D, const float *h, unsigned int L, const float *g,
                            unsigned int Lg, float threshold, ldsp_ambank_t *q);
int ldsp_ambank_destroy(ldsp_ambank_t q);
int ldsp_ambank_reset(ldsp_ambank_t q);
/* Any pointer may be NULL.  skip: input samples per row before the next call's first output. */
int ldsp_ambank_get_info(ldsp_ambank_t q, unsigned int *C, unsigned int *D, unsigned int *L, unsigned int *skip);
int ldsp_ambank_get_taps(ldsp_ambank_t q, float *h, float *g, float *d);   /* L floats each; any may be NULL */
int ldsp_ambank_get_threshold(ldsp_ambank_t q, float *thr);
int ldsp_ambank_set_threshold(ldsp_ambank_t q, float thr);
int ldsp_ambank_num_outputs(ldsp_ambank_t q, size_t K, size_t *ncols);
int ldsp_ambank_execute(ldsp_ambank_t q, const void *x, size_t ldx, size_t K, void *y, size_t ldy, size_t *ncols,
                        int mem, void *stream);
int ldsp_ambank_get_carrier_level(ldsp_ambank_t q, float *level);  /* C floats */
/* Test hook: output columns per workgroup of the (D, L) kernel. */
int ldsp_debug_ambank_tile(unsigned int D, unsigned int L, size_t *frames);

/* ------------------------------------------------------------------------
 * SSBBank: a tuned single-sideband demodulator over the rows of a bank.  Every
 * row of a complex64 [C][K] block (a Channelizer, Downconverter or SquelchBank
 * output) goes to one row of float32 audio, in one launch for all rows; each
 * row has its own beat-frequency oscillator (BFO: the position of the
 * suppressed carrier inside the row) and its own sideband.  The reference's
 * counterpart (ampmodem's SSB modes, SSBDemod here) is one stream per object
 * through a Hilbert filter and cannot be tuned; the definition is this
 * library's own.  With a decimation D, a real low-pass prototype p of L taps, a
 * band (lo, hi) in cycles per row sample measured from the carrier, and for row
 * c a BFO bfo_c in [-0.5, 0.5] and a sideband s_c (+1 upper, -1 lower), with
 * zeros before the stream's start:
 *   w_c      = rint(bfo_c 2^32) mod 2^32                     32-bit BFO word (0.5 is the word of -0.5)
 *   wm       = rint(((lo + hi) / 2) 2^32)                    band-centre word
 *   psi_c[j] = (s_c wm (2j - (L-1)) + 2 j w_c) mod 2^33      integer, counts of 2^-33 turn
 *   g_c[j]   = p[j] exp(2 pi i psi_c[j] / 2^33)              host, double, rounded once to complex64
 *   S[c][n]  = sum_{j<L} g_c[j] x[c][nD - j]
 *   rot_c(n) = exp(-2 pi i ((((nD) mod 2^32) w_c) mod 2^32) / 2^32)   n the absolute 64-bit column index
 *   y[c][n]  = Re(rot_c(n) S[c][n])
 * This equals Re(sum_j q_c[j] v[nD - j]) with v[t] = x[t] exp(-2 pi i t w_c / 2^32)
 * (the carrier moved to DC) and q_c[j] = p[j] exp(2 pi i s_c fm (j - (L-1)/2)),
 * fm = wm / 2^32 (the complex band-pass over the chosen sideband); the split is
 * exact because the phase is additive modulo 2^32, as in the Downconverter.
 * For x = (m(t) + i s m^(t)) exp(2 pi i bfo t), m^ the Hilbert transform of m
 * (liquid's ampmodem SSB convention, gain 1), y is m delayed by (L - 1) / 2
 * input samples.  Nothing is tracked from column to column, there is no AGC,
 * and a row has no serial state but its last L - 1 raw samples.  The rotation
 * is the double sincospi of the exact phase rounded once; S_re = P.x - Q.y and
 * S_im = P.y + Q.x from the four real sums P = sum Re g (x_re, x_im),
 * Q = sum Im g (x_re, x_im), and y = fma(cos, S_re, sin * S_im) + 0 are single
 * float32 operations.  A row of zeros (a block a SquelchBank closed) gives +0.
 * Every row of y is within 1e-6 of the float64 evaluation of the definition
 * from the float32 taps g (max-norm, relative to the row's largest output; for
 * a row whose output is the residue of rejected content, relative to
 * max_n sum_j |g_c[j]| |x[nD - j]|).
 * The column schedule is the Channelizer's and the AMBank's: output n is
 * emitted by the call that delivers sample nD of every row; with T samples per
 * row seen before a call and skip = (-T) mod D, a call of K samples per row
 * returns K > skip ? ceil((K - skip) / D) : 0 columns; calls of any K, 0
 * included, are allowed.  A row's bits depend neither on how the stream is cut
 * into calls, nor on the other rows, their number or order, nor on the row
 * strides.
 *   1 <= C <= 256, fixed at creation;  1 <= D <= 32;  1 <= L <= 1025;
 *   0 < lo < hi <= 0.5 / D;  |bfo_c| <= 0.5;  s_c = +1 or -1;  as > 0.
 * hi = 0 stands for 0.5 / D - lo (LDSP_EINVAL if that leaves hi <= lo).
 * ldsp_ssbbank_create designs, with L = 0 for 2 ceil(1 / lo) + 1 (81 at
 * lo = 0.025: a 60 dB Kaiser's transition is then about 1.8 lo, the band is
 * -6 dB at lo and hi and the stop band begins about 0.1 lo above the carrier,
 * so the carrier and the opposite sideband are both rejected),
 *   p = firdes_kaiser(L, (float)((hi - lo) / 2), as, 0),
 * each tap then divided in double by the double sum of the float32 design and
 * rounded once (unit DC gain).  ldsp_ssbbank_create_taps takes p as given.
 * bfo and sideband have C entries each.  A value out of range (a NaN among
 * them) and a NULL pointer are LDSP_EINVAL; a default L above 1025 (lo below
 * 1 / 512) is LDSP_EUNSUP.
 * ldsp_ssbbank_set_bfo and ldsp_ssbbank_set_sideband take the whole list of C
 * entries and take effect at the next call; the history is raw input and is
 * not touched, and the device tables are replaced once the object's earlier
 * calls have finished.
 * ldsp_ssbbank_execute reads row c at x + c * ldx and writes row c at
 * y + c * ldy (all in samples, ldx >= K): the output is a [C][ncols] image an
 * AudioBank(C, ...) reads in place.  It sets *ncols and, when ldy < *ncols,
 * returns LDSP_ERANGE without consuming the input.  Argument errors are decided
 * on the host before any device work.
 * Not built: independent-sideband output (both sidebands of a row at once),
 * DSB-SC with carrier recovery, a per-row band or decimation, an AGC, an
 * automatic BFO search, skipping closed rows, any change of SSBDemod /
 * HilbertTransform / AMBank / execute_many.
 * ---------------------------------------------------------------------- */
typedef struct ldsp_ssbbank_s *ldsp_ssbbank_t;
/* hi = 0: the default upper edge;  L = 0: the default length. */
int ldsp_ssbbank_create(unsigned int C, unsigned int D, double lo, double hi, unsigned int L, float as,
                        const double *bfo, const int *sideband, ldsp_ssbbank_t *q);
int ldsp_ssbbank_create_taps(unsigned int C, unsigned int D, const float *p, unsigned int L, double lo, double hi,
                             const double *bfo, const int *sideband, ldsp_ssbbank_t *q);
int ldsp_ssbbank_destroy(ldsp_ssbbank_t q);
int ldsp_ssbbank_reset(ldsp_ssbbank_t q);
/* Any pointer may be NULL.  skip: input samples per row before the next call's first output. */
int ldsp_ssbbank_get_info(ldsp_ssbbank_t q, unsigned int *C, unsigned int *D, unsigned int *L, unsigned int *skip);
int ldsp_ssbbank_get_band(ldsp_ssbbank_t q, double *lo, double *hi);       /* either may be NULL */
/* p: L floats;  g: C * L complex64 (re, im), row c's g_c[j] at g[2 (c L + j)];  either may be NULL */
int ldsp_ssbbank_get_taps(ldsp_ssbbank_t q, float *p, float *g);
int ldsp_ssbbank_get_words(ldsp_ssbbank_t q, uint32_t *w);                 /* C words */
int ldsp_ssbbank_get_bfo(ldsp_ssbbank_t q, double *bfo);                   /* C doubles, as given */
int ldsp_ssbbank_set_bfo(ldsp_ssbbank_t q, const double *bfo);             /* C doubles */
int ldsp_ssbbank_get_sideband(ldsp_ssbbank_t q, int *sideband);            /* C ints, +1 or -1 */
int ldsp_ssbbank_set_sideband(ldsp_ssbbank_t q, const int *sideband);      /* C ints, +1 or -1 */
int ldsp_ssbbank_num_outputs(ldsp_ssbbank_t q, size_t K, size_t *ncols);
int ldsp_ssbbank_execute(ldsp_ssbbank_t q, const void *x, size_t ldx, size_t K, void *y, size_t ldy, size_t *ncols,
                         int mem, void *stream);
/* Test hooks: output columns per workgroup of the (D, L) kernel; reset, then stream position T (zero history). */
int ldsp_debug_ssbbank_tile(unsigned int D, unsigned int L, size_t *frames);
int ldsp_debug_ssbbank_seek(ldsp_ssbbank_t q, uint64_t T);

/* ------------------------------------------------------------------------
 * AGCBank: a look-ahead hang AGC over the rows of a bank: float32 [C][K] (an
 * SSBBank, AMBank or FMBank output read in place, an AudioBank's input) or,
 * with cplx = 1, complex64 [C][K].  No reference counterpart (liquid's agc is a
 * per-sample loop over one stream; ldsp_agc_* restates it); the definition is
 * this library's own.  It is chosen so that the per-row recursion is an exact
 * integer max-plus scan: every partition of a row's blocks gives the same bits.
 * All level arithmetic is in integer units of 2^-24 octave of amplitude
 * (Q = 2^24).  A dB value v becomes llrint(v Q / (20 log10 2)) in double: T
 * (target, dB re amplitude 1), Gmax (max_gain) and d (decay per block).
 * FLOOR = -64 Q, CEIL = +64 Q.  Levels are int32; the one product that leaves
 * that range (blocks times d) is int64 and the result saturates at FLOOR.
 * Per row c, for block b = 0, 1, .. of B samples of the row's stream x[t]
 * (t counts from 0 since creation or reset):
 *   a_b       = the largest |x[t]| of the block over its finite samples (a NaN
 *               or Inf sample counts as 0).  Real rows: |x| as float32.  Complex
 *               rows: the square root, in double, of the largest re re + im im
 *               taken in double (the products are exact there: one rounding).
 *   peak_q[b] = clamp(ceil(log2(a_b) Q), FLOOR, CEIL), FLOOR for a_b = 0; log2 in
 *               double, once per block
 *   w_b       = max(peak_q[b - H .. b])              blocks before 0: FLOOR
 *   L_b       = max(w_b, L_{b-1} - d, FLOOR),  L_{-1} = FLOOR
 *             = max(FLOOR, max_{j <= b} (peak_q[j] - d max(0, b - j - H)))
 *               instant attack, a hold of H blocks, then d per block
 *   gain_q[b] = min(T - L_b, Gmax)
 *   g_b       = (float) exp2(gain_q[b] / Q)          exp2 in double, once per block
 *   h_b       = min(g_b, g_{b+1}),  h_{-1} = g_0     boundary gains: one block of look-ahead
 *   y[bB + i] = x[bB + i] gamma,  gamma = h_{b-1} + (h_b - h_{b-1}) (i + 1) / B
 *               in float32, evaluated left to right, i = 0 .. B - 1
 * So gamma <= g_b everywhere in block b and |y| <= target up to float32
 * rounding; the gain ramps and never steps.  A non-finite input sample comes
 * out non-finite at its own position and nowhere else; a row of zeros comes out
 * as zeros at max_gain.  gain_q is an exact function of the peak_q returned.
 * Block b is tracked (peak_q, gain_q) by the call that delivers its last sample
 * and emitted by the call that delivers the last sample of block b + 1: after T
 * samples T / B blocks are tracked and max(0, T / B - 1) emitted.  A call returns
 * the difference of each count; output sample t lines up with input sample t.
 * K = 0 and calls too short for a block are allowed and carry state only.  The
 * object carries per row the up to 2B - 1 samples not yet emitted, the last H
 * quantised peaks, the tracker level and the two boundary gains in flight.  A
 * row's bits (y, peak_q, gain_q) depend neither on how the stream is cut into
 * calls, nor on the other rows, their number or order, nor on the row strides.
 *   1 <= C <= 256;  16 <= B <= 4096 (any integer);  0 <= H <= 255 blocks;
 *   decay >= 0 dB per block (from 128 octaves per block on it acts as that);
 *   |target| and |max_gain| <= 180 dB;  ntarget = 1 (every row) or C.
 * Anything else (a NaN among them) is LDSP_EINVAL.  Everything is fixed at
 * creation.
 * ldsp_agcbank_execute reads row c at x + c * ldx (samples, ldx >= K) and writes
 * row c of the emitted samples to y + c * ldy (samples) and of peak_q and gain_q
 * to peak_q + c * ldq and gain_q + c * ldq (int32).  It sets *nw to the samples
 * written per row and, when ldy < *nw or ldq < the tracked blocks, returns
 * LDSP_ERANGE without consuming the input.  Argument errors are decided on the
 * host before any device work.
 * ldsp_agcbank_get_state copies out, per row, the tracker level, the last H
 * peaks (oldest first) and the two boundary gains (h before the pending block,
 * the pending block's g; 0 before the first block) after the last call; it
 * waits for that call.
 * Not built: a target setter, a flush of the last blocks, a measure-only call,
 * an RMS detector, a per-row block / hang / decay, a sample-rate-aware time
 * constant, skipping closed rows, any change of ldsp_agc_*.
 * ---------------------------------------------------------------------- */
typedef struct ldsp_agcbank_s *ldsp_agcbank_t;
int ldsp_agcbank_create(unsigned int C, unsigned int B, const double *target_dB, unsigned int ntarget, double max_gain_dB,
                        unsigned int hang, double decay_dB, int cplx, ldsp_agcbank_t *q);
int ldsp_agcbank_destroy(ldsp_agcbank_t q);
int ldsp_agcbank_reset(ldsp_agcbank_t q);
/* Any pointer may be NULL.  target_dB: C doubles.  fill: samples per row carried to the next call. */
int ldsp_agcbank_get_info(ldsp_agcbank_t q, unsigned int *C, unsigned int *B, unsigned int *hang, double *decay_dB,
                          double *max_gain_dB, double *target_dB, int *cplx, unsigned int *fill);
/* Blocks a call of K samples tracks and emits; either pointer may be NULL, not both. */
int ldsp_agcbank_num_outputs(ldsp_agcbank_t q, size_t K, size_t *tracked, size_t *emitted);
int ldsp_agcbank_execute(ldsp_agcbank_t q, const void *x, size_t ldx, size_t K, void *y, size_t ldy, int32_t *peak_q,
                         int32_t *gain_q, size_t ldq, size_t *nw, int mem, void *stream);
/* Any pointer may be NULL.  level: C;  peaks: C * H;  gains: C * 2. */
int ldsp_agcbank_get_state(ldsp_agcbank_t q, int32_t *level, int32_t *peaks, float *gains);
/* Test hooks: dB to units;  the tracker on the host: L[i] for n new peaks in
 * partitions of `width` blocks, from *level (updated) and the `hang` peaks
 * before them (oldest first, updated), with the decay d in units. */
int ldsp_debug_agcbank_units(double dB, int64_t *units);
int ldsp_debug_agcbank_track(const int32_t *peak_q, size_t n, unsigned int hang, int64_t d, size_t width, int32_t *level,
                             int32_t *peaks, int32_t *L);

/* ------------------------------------------------------------------------
 * ToneBank: for every row of a float32 [C][K] block (an FMBank, AMBank, SSBBank
 * or AGCBank output, read in place), the power at F listed tones per block of B
 * samples, the dominant tone of the block and, optionally, the rows themselves
 * with the blocks zeroed in which no accepted tone was heard lately: a CTCSS /
 * tone-burst / paging-tone detector and tone squelch.  No reference counterpart;
 * the definition is this library's own.  The F tones f_k (cycles per row sample)
 * are common to all rows.  With the window w[i] = 0.5 - 0.5 cos(2 pi i / B)
 * (HANN, periodic) or 1 (RECT) and s = sqrt(2) / sum_i w[i], the tables
 *   Tc[k][i] = s w[i] cos(2 pi f_k i)      Ts[k][i] = -s w[i] sin(2 pi f_k i)
 * are computed in double and each entry rounded once to float32; the phase
 * restarts at every block and the kernel multiplies by nothing else.  For block
 * b of row c of the concatenated input x[c][t] (t counted from 0 since creation
 * or reset):
 *   Xre = sum_{i<B} Tc[k][i] x[c][bB + i]   Xim = sum_{i<B} Ts[k][i] x[c][bB + i]
 *   power[c][b][k] = fmaf(Xre, Xre, Xim * Xim)                          float32
 * Xre and Xim are float32 values whose summation order is fixed by B alone:
 * float32 fmaf chains over S = 16, 32, 64, 128, 256 samples each (from B = 64,
 * 256, 1024, 4096, 16384 up), whose sums are added in float64 in a fixed order
 * and rounded once to float32 (one chain over 192 samples measured 1.2e-6 of
 * the largest power off, over 4096 samples 2.4e-6 emulated).  A sinusoid of
 * amplitude A at f_k reads A^2 / 2.  Two tones closer than 2 / B cycles per
 * sample (HANN; 1 / B for RECT) both respond to either.  The decision is an
 * exact function of the float32 powers returned:
 *   k* = the lowest index of the block's largest power
 *   others = sum_{k != k*} (double) power[k], added in index order
 *   hit = every power of the block is finite
 *         and power[k*] > floor                              (in float32)
 *         and (double) power[k*] (F - 1) > dominance others  (in float64)
 *   tone[c][b] = hit ? k* : -1                                             int8
 *   accepted = hit and (want[c] < 0 or want[c] == k*)
 *   open[c][b] = some block in [b - hold, b] of the row's stream was accepted
 *                (blocks before the stream's start were not)        uint8, 0 / 1
 *   y[c][bB + i] = open ? x[c][bB + i] (the same bits) : +0.0
 * The compares are strict: a block of zeros is never a hit.  dominance is the
 * ratio of the best power to the mean of the others.
 * Block b is emitted by the call that delivers its last sample, as the
 * SquelchBank's: with T samples per row seen before a call, a call of K samples
 * returns (T + K) / B - T / B blocks; K = 0 and calls too short for a block carry
 * state only; the fill = (T + K) mod B samples of the unfinished block are
 * carried, and the gated output of a call is float32 [C][nblocks B].  Per-row
 * state is the carried samples and one integer, the blocks since the last
 * accepted one, which saturates at 65.  A row's bits (power, tone, open, gated
 * samples) depend neither on how the stream is cut into calls, nor on the other
 * rows, their number or order, nor on the row strides.
 *   1 <= C <= 256;  2 <= F <= 64;  0 < f_k < 0.5, finite;  B a multiple of 64,
 *   64 <= B <= 16384;  window LDSP_TONE_RECT or LDSP_TONE_HANN;  dominance >= 1;
 *   floor >= 0;  0 <= hold <= 64;  -1 <= want[c] <= F - 1 (-1: any listed tone).
 * Anything else (a NaN among them) is LDSP_EINVAL.  Argument errors are decided
 * on the host before any device work.
 * ldsp_tonebank_create sets want = -1 for every row.  ldsp_tonebank_set_want
 * takes n = 1 (every row) or n = C values; it, ldsp_tonebank_set_dominance and
 * ldsp_tonebank_set_floor take effect at the next block and touch no state;
 * ldsp_tonebank_reset restores the initial state and keeps the settings.
 * ldsp_tonebank_execute reads row c at x + c * ldx (ldx >= K) and writes row c
 * of power to power + c * ldp (floats, [nblocks][F]), of tone to tone + c * ldt,
 * of open to open + c * ldo (bytes; open may be NULL) and, where y is not NULL,
 * of the gated samples to y + c * ldy; with y == NULL it only measures.  It
 * sets *nblocks and, when ldp < *nblocks F, ldt or ldo < *nblocks or ldy <
 * *nblocks B, returns LDSP_ERANGE without consuming the input.
 * ldsp_tonebank_get_state copies out, per row, the blocks since the last
 * accepted one (65: none within reach); it waits for the last call.
 * Not built: overlapping blocks, a look-ahead block (a transmission's first
 * partial block stays closed), complex rows, per-row tone lists, blocks or
 * thresholds, DTMF pair logic, code (DCS) squelch, skipping closed rows.
 * ---------------------------------------------------------------------- */
typedef struct ldsp_tonebank_s *ldsp_tonebank_t;
enum { LDSP_TONE_RECT = 0, LDSP_TONE_HANN = 1 };
int ldsp_tonebank_create(unsigned int C, const double *tones, unsigned int F, unsigned int B, int window,
                         double dominance, float floor, unsigned int hold, ldsp_tonebank_t *q);
int ldsp_tonebank_destroy(ldsp_tonebank_t q);
int ldsp_tonebank_reset(ldsp_tonebank_t q);
/* Any pointer may be NULL.  fill: samples per row carried to the next call. */
int ldsp_tonebank_get_info(ldsp_tonebank_t q, unsigned int *C, unsigned int *F, unsigned int *B, int *window,
                           unsigned int *hold, unsigned int *fill);
/* Any pointer may be NULL.  tones: F;  tc, ts: F * B each, [k][i];  sumw: sum_i w[i] in double. */
int ldsp_tonebank_get_tables(ldsp_tonebank_t q, double *tones, float *tc, float *ts, double *sumw);
int ldsp_tonebank_set_want(ldsp_tonebank_t q, const int *want, unsigned int n);     /* n = 1 or C */
int ldsp_tonebank_get_want(ldsp_tonebank_t q, int *want);                           /* C values */
int ldsp_tonebank_set_dominance(ldsp_tonebank_t q, double dominance);
int ldsp_tonebank_get_dominance(ldsp_tonebank_t q, double *dominance);
int ldsp_tonebank_set_floor(ldsp_tonebank_t q, float floor);
int ldsp_tonebank_get_floor(ldsp_tonebank_t q, float *floor);
int ldsp_tonebank_num_outputs(ldsp_tonebank_t q, size_t K, size_t *nblocks);
int ldsp_tonebank_execute(ldsp_tonebank_t q, const float *x, size_t ldx, size_t K, float *power, size_t ldp, int8_t *tone,
                          size_t ldt, uint8_t *open, size_t ldo, float *y, size_t ldy, size_t *nblocks, int mem,
                          void *stream);
int ldsp_tonebank_get_state(ldsp_tonebank_t q, int *since);                         /* C values */
/* Test hook: columns (row, block pairs) per workgroup of the power kernel. */
int ldsp_debug_tonebank_tile(unsigned int B, size_t *columns);

/* ------------------------------------------------------------------------
 * Spectrogram: a streaming Welch periodogram, one complex64 stream to rows of
 * power per bin and a running mean of them.  No reference counterpart
 * (liquid's spgramcf / spwaterfallcf are the same block: a zeroed window
 * buffer and a transform every `delay` pushes); the definition is this
 * library's own.  The stream x[t] counts t from 0 since creation or reset,
 * with zeros before t = 0; N = nfft, a window w of W taps (1 <= W <= N), a hop
 * d (1 <= d <= W) and A >= 1 transforms per row.  Transform s = 0, 1, .. is
 * taken when sample t = (s + 1) d - 1 arrives:
 *   X_s[k] = sum_{i<W} w[i] x[(s + 1) d - W + i] exp(-2 pi i k i / N)    k < N
 *   P_s[k] = re(X_s[k])^2 + im(X_s[k])^2
 *   row r  = (1 / A) sum_{s = rA}^{rA + A - 1} P_s
 *   psd    = (1 / S) sum P_s over the S transforms since create / reset / clear
 * The windowed samples are FFT inputs 0 .. W - 1, zero-padded to N.  Bins are
 * in FFT order: bin k is at k / N cycles per sample, k >= N / 2 the negative
 * frequencies.  With T samples seen before a call of n samples the call takes
 * floor((T + n) / d) - floor(T / d) transforms and returns the rows whose last
 * transform it delivers: floor(s1 / A) - floor(s0 / A) with s0, s1 the
 * transform counts since create / reset before and after (clear does not move
 * the row schedule).  Calls of any length, 0 included, are allowed, and a
 * row's bits do not depend on how the stream is cut into calls.
 * Named windows (t = i / (W - 1); W = 1 gives w = [1]) are computed in double,
 * normalised in double to unit noise gain, sum w[i]^2 = 1 (white noise of
 * variance v reads v in every bin), and rounded once to float32:
 *   RECT 1;  HANN 0.5 - 0.5 cos 2 pi t;  HAMMING 0.53836 - 0.46164 cos 2 pi t;
 *   BLACKMANHARRIS 0.35875 - 0.48829 cos 2 pi t + 0.14128 cos 4 pi t
 *                  - 0.01168 cos 6 pi t
 * ldsp_spgram_create_window takes w as given (not normalised).
 *   N not a power of two, W = 0, W > N, d = 0, A = 0, an unknown wtype:
 *   LDSP_EINVAL;  a power-of-two N below 256 or above 4096, d > W: LDSP_EUNSUP.
 * ldsp_spgram_execute writes row r to y + r * ld (ld in floats, >= nfft, else
 * LDSP_EINVAL); y = NULL accumulates only (ld is ignored, *nrows still set).
 * ldsp_spgram_get_psd copies the mean to a host array of nfft doubles (zeros
 * while S = 0) and synchronises.  ldsp_spgram_clear zeroes the accumulator and
 * S only; ldsp_spgram_reset also the history, T and the unfinished row.  The
 * accumulator is float64 on the device and is added to in a fixed order: the
 * same sequence of calls gives the same bits, with or without row stores.
 * Argument errors are decided on the host before any device work.
 * Not built: exponential averaging, real input, d > W, dB output, fftshift.
 * ---------------------------------------------------------------------- */
typedef struct ldsp_spgram_s *ldsp_spgram_t;
enum { LDSP_WIN_RECT = 0, LDSP_WIN_HANN = 1, LDSP_WIN_HAMMING = 2, LDSP_WIN_BLACKMANHARRIS = 3 };
int ldsp_spgram_create(unsigned int nfft, int wtype, unsigned int W, unsigned int d, unsigned int A,
                       ldsp_spgram_t *q);
int ldsp_spgram_create_window(unsigned int nfft, const float *w, unsigned int W, unsigned int d, unsigned int A,
                              ldsp_spgram_t *q);
int ldsp_spgram_destroy(ldsp_spgram_t q);
int ldsp_spgram_reset(ldsp_spgram_t q);
int ldsp_spgram_clear(ldsp_spgram_t q);
/* Any output pointer may be NULL.  samples: T; transforms: S. */
int ldsp_spgram_get_info(ldsp_spgram_t q, unsigned int *nfft, unsigned int *W, unsigned int *d, unsigned int *A,
                         uint64_t *samples, uint64_t *transforms);
int ldsp_spgram_get_window(ldsp_spgram_t q, float *w);           /* W floats */
int ldsp_spgram_num_outputs(ldsp_spgram_t q, size_t n, size_t *ntransforms, size_t *nrows);
int ldsp_spgram_execute(ldsp_spgram_t q, const void *x, size_t n, float *y, size_t ld, size_t *nrows, int mem,
                        void *stream);
/* ldsp_bytes_to_iq fused into the transform's loads, as ldsp_chan_execute_iq16:
 * x holds n native int16 (I, Q) pairs (4 n bytes, 4-byte aligned); the checks,
 * *nrows, the rows, the accumulator's bits and the state after the call are
 * those of ldsp_bytes_to_iq followed by ldsp_spgram_execute. */
int ldsp_spgram_execute_iq16(ldsp_spgram_t q, const void *x, size_t n, float *y, size_t ld, size_t *nrows, int mem,
                             void *stream);
int ldsp_spgram_get_psd(ldsp_spgram_t q, double *psd, uint64_t *transforms);
/* Test hook: transforms per workgroup of the nfft kernel (at A > 1: whole rows, at least one). */
int ldsp_debug_spgram_tile(unsigned int nfft, size_t *transforms);

/* ------------------------------------------------------------------------
 * Raw IQ conversion. Replaces bytes_to_iq (src/utility.hpp:61-69,
 * wrapper.cpp:13): interleaved native int16 (I, Q) -> complex64 / 32767.
 * nbytes / 4 samples are converted (a trailing partial sample is ignored).
 * ---------------------------------------------------------------------- */
int ldsp_bytes_to_iq(const void *in, size_t nbytes, void *y, int mem, void *stream);

/* ------------------------------------------------------------------------
 * Many-calls: one call each on C independent objects of one class (no
 * reference counterpart -- the reference's SDR callback runs one channel's
 * chain per call, README.md:53-58; SURVEY 7 H5 / 8(e): channels batched on one
 * GPU).  Equivalent to calling the single-object execute on q[0], .., q[C-1]
 * in turn on `stream`, bit for bit, but every kernel runs as ONE launch for
 * all objects that take the same path (blockIdx.y = object), so a step of C
 * channels issues as many launches as one channel's.  Device pointers only;
 * all objects get n input samples; the objects must be distinct.
 * iirfilt_resamp: nout[c] receives object c's output count (cap per object).
 * ---------------------------------------------------------------------- */
int ldsp_agc_execute_many(ldsp_agc_t *q, const void *const *x, size_t n, void *const *y, int C, void *stream);
int ldsp_ampmodem_demodulate_many(ldsp_ampmodem_t *q, const void *const *x, size_t n, void *const *y, int C,
                                  void *stream);
int ldsp_iirfilt_execute_many(ldsp_iirfilt_t *q, const void *const *x, size_t n, void *const *y, int C,
                              void *stream);
int ldsp_iirfilt_resamp_execute_many(ldsp_iirfilt_t *q, ldsp_resamp_t *rs, const void *const *x, size_t n,
                                     void *const *y, size_t cap, size_t *nout, int C, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LDSP_H */
