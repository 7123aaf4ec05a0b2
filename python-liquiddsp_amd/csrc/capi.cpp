// capi.cpp -- the C ABI of libldsp (include/ldsp.h): object lifetime, host-side
// design and state bookkeeping, device staging, and dispatch to the gfx950
// kernels.  No CPU fallback exists: every execute runs on a HIP device and
// fails with LDSP_EHIP when none is present.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <math.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iterator>
#include <map>
#include <set>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "agc_track.hpp"
#include "batch.hpp"
#include "design.hpp"
#include "modal.hpp"
#include "kernels.hpp"
#include "ldsp_math.hpp"
#include "ldsp_common.hpp"

namespace ldsp {

static thread_local std::string g_last_error;

#ifdef LDSP_TUNING
long knob_env(const char* name, long dflt)
{
    const char* v = std::getenv(name);
    return v ? std::atol(v) : dflt;
}
double knob_env_f(const char* name, double dflt)
{
    const char* v = std::getenv(name);
    return v ? std::atof(v) : dflt;
}
const char* knob_env_s(const char* name) { return std::getenv(name); }
#endif
void set_last_error(const std::string& m) { g_last_error = m; }

// roctx through dlopen (ldsp_common.hpp RoctxRange): resolved once; absent library -> no-ops
namespace {
struct Roctx {
    int (*push)(const char*) = nullptr;
    int (*pop)() = nullptr;
    Roctx()
    {
        void* h = nullptr;
        for (const char* name : {"librocprofiler-sdk-roctx.so.1", "librocprofiler-sdk-roctx.so",
                                 "/opt/rocm/lib/librocprofiler-sdk-roctx.so.1"}) {
            if ((h = dlopen(name, RTLD_NOW | RTLD_LOCAL)) != nullptr) break;
        }
        if (!h) return;
        push = (int (*)(const char*))dlsym(h, "roctxRangePushA");
        pop = (int (*)())dlsym(h, "roctxRangePop");
        if (!push || !pop) push = nullptr, pop = nullptr;
    }
};
const Roctx& roctx()
{
    static const Roctx r;
    return r;
}
} // namespace
void roctx_push(const char* m)
{
    if (roctx().push) roctx().push(m);
}
void roctx_pop()
{
    if (roctx().pop) roctx().pop();
}

int current_device()
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0) throw Error(LDSP_EHIP, "no HIP device available (libldsp has no CPU fallback)");
    int d = 0;
    LDSP_HIP(hipGetDevice(&d));
    return d;
}

hipStream_t library_stream(int device)
{
    static std::mutex mu;
    static std::vector<hipStream_t> streams;
    std::lock_guard<std::mutex> lk(mu);
    if ((int)streams.size() <= device) streams.resize(device + 1, nullptr);
    if (!streams[device]) {
        DeviceGuard g(device);
        LDSP_HIP(hipStreamCreateWithFlags(&streams[device], hipStreamNonBlocking));
    }
    return streams[device];
}

// Resolve where a call runs: host-memory calls use the library stream and stage
// through grow-only device buffers owned by the object.
struct Exec {
    int device;
    hipStream_t stream;
    bool host;
};

// The device a call's buffers live on.  A device-memory call runs on the
// device that holds its input (made current for the call, so an object's first
// call binds it there); a host-memory call on the current device.
struct BufDevice {
    int dev;
    DeviceGuard g;
    static int of(int mem, const void* x)
    {
        if (mem == LDSP_MEM_DEVICE && x) {
            hipPointerAttribute_t a;
            if (hipPointerGetAttributes(&a, x) == hipSuccess && a.type == hipMemoryTypeDevice) return a.device;
            (void)hipGetLastError();
        }
        return current_device();
    }
    BufDevice(int mem, const void* x) : dev(of(mem, x)), g(dev) {}
};

static int checked_mem(int mem)
{
    LDSP_REQUIRE(mem == LDSP_MEM_HOST || mem == LDSP_MEM_DEVICE, "mem must be LDSP_MEM_HOST or LDSP_MEM_DEVICE");
    return mem;
}

static Exec make_exec(int device, int mem, void* stream, const BufDevice& bd)
{
    if (mem == LDSP_MEM_DEVICE && bd.dev != device)
        throw Error(LDSP_EINVAL, "buffer on device " + std::to_string(bd.dev) + " but the object lives on device " +
                                     std::to_string(device) + " (objects are bound to the device of their first call)");
    Exec e;
    e.device = device;
    e.host = (mem == LDSP_MEM_HOST);
    e.stream = e.host ? library_stream(device) : (hipStream_t)stream;
    return e;
}

template <typename T>
static T* upload(DevBuf& b, const std::vector<T>& v, int dev)
{
    b.ensure(std::max<size_t>(v.size(), 1) * sizeof(T), dev);
    if (!v.empty()) LDSP_HIP(hipMemcpy(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return b.as<T>();
}

// Zero device memory before any stream can read it: hipMemset runs on the
// null stream, which does not order against the non-blocking library stream or
// a caller's stream, so wait for it (create / reset paths only).
static void zero_now(void* p, int v, size_t bytes)
{
    LDSP_HIP(hipMemset(p, v, bytes));
    LDSP_HIP(hipDeviceSynchronize());
}

// Host <-> device staging for LDSP_MEM_HOST calls
// Host buffers pass through a pinned staging buffer (a copy from / to pageable
// memory is staged by the runtime at a fraction of the DMA rate, and it is the
// per-call overhead of the README's numpy callbacks); each host call ends with a
// stream synchronize, so the next call may reuse the buffer.  Above kPinMax the
// pageable copy is used directly (no pinned memory of that size per object).
struct PinnedBuf {
    void* p = nullptr;
    size_t cap = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    ~PinnedBuf() {
        if (p) (void)hipHostFree(p);
    }
    void* ensure(size_t bytes) {
        if (bytes <= cap && p) return p;
        const size_t want = (std::max(bytes, cap + cap / 4) + 65535) & ~(size_t)65535;
        if (p) LDSP_HIP(hipHostFree(p));
        p = nullptr;
        cap = 0;
        LDSP_HIP(hipHostMalloc(&p, want, hipHostMallocDefault));
        cap = want;
        return p;
    }
};
// Host staging of the numpy (host-buffer) path: pinned buffers shared by every
// object a thread calls on one device (a host-buffer call is synchronous -- it
// returns only after its output copy -- so a thread's calls never overlap in
// them).  Grown on demand up to kPinMax each (larger transfers go unpinned), never
// shrunk.  A thread takes a pool from a process-wide free list on its first host
// call on a device and returns it there when it exits (thread_local holder), so
// short-lived threads (thread pools, DataLoader workers) reuse pools instead of
// leaking page-locked memory: the number of pools is bounded by the number of
// threads making host calls at the same time.  The free list itself is never
// destroyed (hipHostFree at process teardown can outlive the HIP runtime).
struct PinnedPool {
    PinnedBuf hin, hout;
    hipEvent_t hin_done = nullptr;    // the last copy out of hin (a call that threw may not have synchronized)
    hipEvent_t done()
    {
        if (!hin_done) LDSP_HIP(hipEventCreateWithFlags(&hin_done, hipEventDisableTiming));
        return hin_done;
    }
};
namespace {
struct PoolList {
    std::mutex mu;
    std::vector<std::vector<PinnedPool*>> free;    // per device
    size_t total = 0;                              // pools ever created
};
PoolList& pool_list()
{
    static PoolList* l = new PoolList();           // never destroyed (see above)
    return *l;
}
struct ThreadPools {
    std::vector<PinnedPool*> pools;                // this thread's, per device
    ~ThreadPools()
    {
        PoolList& l = pool_list();
        std::lock_guard<std::mutex> lk(l.mu);
        for (size_t d = 0; d < pools.size(); d++)
            if (pools[d]) {
                if (l.free.size() <= d) l.free.resize(d + 1);
                l.free[d].push_back(pools[d]);
            }
    }
};
} // namespace
static PinnedPool& pinned_pool(int device)
{
    thread_local ThreadPools tp;
    if ((int)tp.pools.size() <= device) tp.pools.resize(device + 1, nullptr);
    if (!tp.pools[device]) {
        PoolList& l = pool_list();
        std::lock_guard<std::mutex> lk(l.mu);
        if ((int)l.free.size() > device && !l.free[device].empty()) {
            tp.pools[device] = l.free[device].back();
            l.free[device].pop_back();
        } else {
            tp.pools[device] = new PinnedPool();
            l.total++;
        }
    }
    return *tp.pools[device];
}

// Is p page-locked host memory (ldsp_host_alloc, hipHostMalloc, hipHostRegister)?
// Such buffers are copied by DMA directly (no staging copy on the host).
static bool host_pinned(const void* p)
{
    if (!p) return false;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) == hipSuccess) return a.type == hipMemoryTypeHost;
    (void)hipGetLastError();
    return false;
}

struct Staging {
    static constexpr size_t kPinMax = (size_t)16 << 20;
    DevBuf in, out;                   // per object (device side)
    Staging() = default;
    Staging(const Staging&) = delete;
    Staging& operator=(const Staging&) = delete;
    const void* dev_in(const Exec& e, const void* x, size_t bytes)
    {
        if (!e.host) return x;
        in.ensure(bytes, e.device);
        if (bytes && host_pinned(x)) {
            // page-locked input: DMA from it directly (the call ends with a synchronize)
            LDSP_HIP(hipMemcpyAsync(in.p, x, bytes, hipMemcpyHostToDevice, e.stream));
        } else if (bytes && bytes <= kPinMax) {
            PinnedPool& pp = pinned_pool(e.device);
            LDSP_HIP(hipEventSynchronize(pp.done()));
            std::memcpy(pp.hin.ensure(bytes), x, bytes);
            LDSP_HIP(hipMemcpyAsync(in.p, pp.hin.p, bytes, hipMemcpyHostToDevice, e.stream));
            LDSP_HIP(hipEventRecord(pp.hin_done, e.stream));
        } else if (bytes) {
            LDSP_HIP(hipMemcpyAsync(in.p, x, bytes, hipMemcpyHostToDevice, e.stream));
        }
        return in.p;
    }
    void* dev_out(const Exec& e, void* y, size_t bytes)
    {
        if (!e.host) return y;
        return out.ensure(bytes, e.device);
    }
    void finish(const Exec& e, void* y, size_t bytes)
    {
        if (!e.host) return;
        if (bytes && host_pinned(y)) {
            LDSP_HIP(hipMemcpyAsync(y, out.p, bytes, hipMemcpyDeviceToHost, e.stream));
            PinnedPool& pp = pinned_pool(e.device);
            LDSP_HIP(hipEventRecord(pp.done(), e.stream));
            LDSP_HIP(hipEventSynchronize(pp.done()));
            return;
        }
        if (bytes && bytes <= kPinMax) {
            PinnedPool& pp = pinned_pool(e.device);
            LDSP_HIP(hipMemcpyAsync(pp.hout.ensure(bytes), out.p, bytes, hipMemcpyDeviceToHost, e.stream));
            // wait on an event (the host spins on it) rather than the stream, whose
            // synchronize may yield the thread: a README block makes five of these waits
            LDSP_HIP(hipEventRecord(pp.done(), e.stream));
            LDSP_HIP(hipEventSynchronize(pp.hin_done));
            std::memcpy(y, pp.hout.p, bytes);
            return;
        }
        if (bytes) LDSP_HIP(hipMemcpyAsync(y, out.p, bytes, hipMemcpyDeviceToHost, e.stream));
        LDSP_HIP(hipStreamSynchronize(e.stream));
    }
    // A host image of `rows` rows of `row` bytes whose rows are `stride` bytes
    // apart; the device image is dense.  Dense host images take the paths above.
    const void* dev_in(const Exec& e, const void* x, size_t row, size_t rows, size_t stride)
    {
        if (!e.host || stride == row || row * rows == 0) return dev_in(e, x, row * rows);
        in.ensure(row * rows, e.device);
        LDSP_HIP(hipMemcpy2DAsync(in.p, row, x, stride, row, rows, hipMemcpyHostToDevice, e.stream));
        return in.p;
    }
    void finish(const Exec& e, void* y, size_t row, size_t rows, size_t stride)
    {
        if (!e.host || stride == row || row * rows == 0) return finish(e, y, row * rows);
        LDSP_HIP(hipMemcpy2DAsync(y, stride, out.p, row, row, rows, hipMemcpyDeviceToHost, e.stream));
        LDSP_HIP(hipStreamSynchronize(e.stream));
    }
};

// Streaming state on the device is ping-ponged between two buffers, so a call
// never reads what it writes: it reads in(), writes out() and then flips.
struct PingPong {
    DevBuf b[2];
    int cur = 0;
    void* in() const { return b[cur].p; }
    void* out() const { return b[1 - cur].p; }
    void flip() { cur = 1 - cur; }
    void zero(size_t bytes, int dev)
    {
        for (auto& d : b) zero_now(d.ensure(bytes, dev), 0, bytes);
        cur = 0;
    }
};

// What every object that keeps state on a device has.  An object lives on the
// device of its first call: bind_first() runs the object's own bind(dev) -- its
// uploads and zeroed state, on `dev`, which the caller has made current -- and
// records the device only after bind() returned, so a bind that threw leaves
// the object unbound and its next call binds again.
struct DevObj {
    int device = -1;                  // -1: not bound yet
    hipStream_t last = nullptr;       // the stream of the last call
    StreamMark ord;                   // cross-stream call order (ldsp_common.hpp)
    Staging stg;
    template <class T>
    static int bind_first(T& o, int dev)
    {
        if (o.device < 0) {
            o.bind(dev);
            o.device = dev;
        }
        return o.device;
    }
    // everything the object has enqueued is done
    void quiesce() const
    {
        if (last) LDSP_HIP(hipStreamSynchronize(last));
        ord.sync();
    }
    void drain() const                // a destroy: the last call's stream only, and no error to report
    {
        if (last) (void)hipStreamSynchronize(last);
    }
    // reset-type paths: nothing before the first call; after it, `fn` runs with
    // the object's device current and the object idle
    template <class F>
    void at_rest(F&& fn)
    {
        if (device < 0) return;
        DeviceGuard g(device);
        quiesce();
        fn();
    }
};

// One execute call on an object: validates `mem` (before any HIP call), makes
// the device of buffer `x` current, binds the object there on its first call,
// makes the object's device current, resolves the stream (`e`), and orders the
// call after the object's previous one; end() marks the call's end for the
// next.  ordered == false leaves `ord` to the caller, for objects whose calls
// order their parts themselves.
struct Call {
    DevObj& o;
    const bool ordered;
    const BufDevice bd;
    const DeviceGuard g;
    const Exec e;
    template <class T>
    Call(T& obj, int mem, const void* x, void* stream, bool ordered_ = true)
        : Call(obj, [&](int dev) { return DevObj::bind_first(obj, dev); }, mem, x, stream, ordered_)
    {
    }
    // a call on two objects: both bind under the buffer's device and must share one (`differ`: the message if not)
    template <class T, class U>
    Call(T& obj, U& second, const char* differ, int mem, const void* x, void* stream, bool ordered_ = true)
        : Call(obj,
               [&](int dev) {
                   DevObj::bind_first(obj, dev);
                   DevObj::bind_first(second, dev);
                   LDSP_REQUIRE(obj.device == second.device, differ);
                   return obj.device;
               },
               mem, x, stream, ordered_)
    {
    }
    void end()
    {
        if (ordered) o.ord.mark(e.stream);
        o.last = e.stream;
    }

private:
    template <class B>
    Call(DevObj& obj, B&& bind, int mem, const void* x, void* stream, bool ordered_)
        : o(obj), ordered(ordered_), bd(checked_mem(mem), x), g(bind(bd.dev)), e(make_exec(o.device, mem, stream, bd))
    {
        if (ordered) o.ord.wait(e.stream);
    }
};

// a nested C-ABI call's failure, passed on with its message
static void ok(int rc)
{
    if (rc != LDSP_OK) throw Error(rc, g_last_error);
}

// every destroy: the object's last call has finished with its buffers
template <class T>
static void destroy(T* q)
{
    if (q) q->drain();
    delete q;
}

// ====================================================================== FIR
struct FirObj : DevObj {
    std::vector<float> h;
    bool cplx = false;
    float scale = 1.0f;
    int mode = LDSP_MODE_FAST;
    DevBuf taps_pad, taps_rev;
    PingPong hist;
    DevBuf fft_H, fft_tw;             // overlap-save spectrum (for fft_scale) and twiddles
    DevBuf mixbuf;                    // ldsp_nco_mix_firfilt off the fused path: the mixed samples
    float fft_scale = 0.0f;
    bool fft_ready = false;
    size_t esz() const { return cplx ? 8 : 4; }
    size_t hist_bytes() const { return std::max<size_t>(h.size() - 1, 1) * esz(); }
    // FAST on complex data with L in [kFirFftMinTaps, 513] (fft_P() <= 512) runs
    // the overlap-save FFT kernel (HBM-bound); shorter and longer filters and
    // DIRECT use the register-blocked direct form (VALU-bound at 4 L flop / sample).
    static constexpr int kFirFftMinTaps = 48;
    int fft_P() const { return ((int)h.size() - 1 + 63) / 64 * 64; }
    bool use_fft() const
    {
        const int L = (int)h.size();
        return mode == LDSP_MODE_FAST && cplx && L >= kFirFftMinTaps && fft_P() <= 512;
    }
    // the kernel a call of n samples runs (fir_dispatch, ldsp_debug_fir_dispatch)
    enum Kernel { kDirect = 0, kFft = 1, kExact = 2 };
    Kernel kernel_for(size_t n) const
    {
        if (mode == LDSP_MODE_EXACT) return kExact;
        return use_fft() && n > 0 ? kFft : kDirect;
    }
    void prepare_fft()
    {
        if (fft_ready && fft_scale == scale) return;
        const int L = (int)h.size();
        const int N = k::fir_fft_points(fft_P());
        std::vector<float> Hf(2 * (size_t)N);
        for (int f = 0; f < N; f++) {
            double re = 0.0, im = 0.0;
            for (int i = 0; i < L; i++) {
                const double a = -2.0 * M_PI * (double)(((long)f * i) % N) / N;
                re += (double)h[i] * cos(a);
                im += (double)h[i] * sin(a);
            }
            Hf[2 * f] = (float)(re * (double)scale / N);
            Hf[2 * f + 1] = (float)(im * (double)scale / N);
        }
        // Stockham twiddles exp(-2 pi i r k / (Ns R)), [pass][r-1][k] (kernels.hpp)
        std::vector<float> tw;
        const int p512[2][2] = {{8, 8}, {64, 8}}, p1024[2][2] = {{16, 16}, {256, 4}};
        for (const auto& pr : (N == 512 ? p512 : p1024))
            for (int r = 1; r < pr[1]; r++)
                for (int kk = 0; kk < pr[0]; kk++) {
                    const double a = -2.0 * M_PI * (double)(r * kk) / (double)(pr[0] * pr[1]);
                    tw.push_back((float)cos(a));
                    tw.push_back((float)sin(a));
                }
        upload(fft_H, Hf, device);
        upload(fft_tw, tw, device);
        fft_scale = scale;
        fft_ready = true;
    }
    void bind(int dev)
    {
        const int L = (int)h.size();
        std::vector<float> pad((L + 15) / 16 * 16, 0.0f), rev(L);
        for (int i = 0; i < L; i++) {
            pad[i] = h[i];
            rev[L - 1 - i] = h[i];
        }
        upload(taps_pad, pad, dev);
        upload(taps_rev, rev, dev);
        hist.zero(hist_bytes(), dev);
    }
};
} // namespace ldsp

struct ldsp_firfilt_s : ldsp::FirObj {};
struct ldsp_resamp_s;
struct ldsp_nco_s;
struct ldsp_iirfilt_s;
struct ldsp_agc_s;
struct ldsp_ampmodem_s;

namespace ldsp {

// ====================================================================== resampler
struct ResampObj : DevObj {
    bool cplx = true;                 // complex samples
    bool real_taps = false;           // crcf: complex samples, real taps (CResampler)
    float rate = 1.0f;
    unsigned int m = 0, npfb = 0, sub_len = 0;
    int bits_index = 0;
    uint32_t step = 0;
    uint64_t phase = 0;
    float fc = 0, as = 0;
    std::vector<float> hproto, sub;   // sub: [npfb][sub_len] reversed (complex interleaved if cplx)
    DevBuf dsub;
    PingPong hist;
    size_t esz() const { return cplx ? 8 : 4; }
    size_t hist_bytes() const { return std::max<size_t>(sub_len - 1, 1) * esz(); }
    void set_rate(float r)
    {
        LDSP_REQUIRE(r > 0, "resamp: resampling rate must be greater than zero");
        LDSP_REQUIRE(r >= 0.004f && r <= 250.0f, "resamp: resampling rate must be in [0.004, 250]");
        rate = r;
        step = (uint32_t)round((double)((float)(1 << 24) / rate));
    }
    size_t num_outputs(size_t n) const
    {
        if (n == 0) return 0;
        const long long num = (long long)(n - 1) * (1LL << 24) + 0xffffffLL - (long long)phase;
        return num < 0 ? 0 : (size_t)(num / step) + 1;
    }
    // the plan of the next call of n samples (ldsp_resamp_execute, ldsp_debug_resamp_dispatch)
    k::ResampPlan plan(size_t n) const
    {
        k::ResampPlan p;
        p.P0 = phase;
        p.step = step;
        p.bits_index = bits_index;
        p.sub_len = (int)sub_len;
        p.npfb = (int)npfb;
        p.K = num_outputs(n);
        k::resamp_plan(p, cplx, real_taps);
        return p;
    }
    void bind(int dev)
    {
        upload(dsub, sub, dev);
        hist.zero(hist_bytes(), dev);
    }
};

// ====================================================================== NCO
// (its state is the host's phase words: its calls mark no order, `ord` and `last` stay unset)
struct NcoObj : DevObj {
    int type = 0;
    uint32_t theta = 0, dtheta = 0;
    float alpha = 0.1f, beta = 0.0f;
    std::vector<float> table;
    DevBuf dtab;
    void bind(int dev) { upload(dtab, table, dev); }
};

static std::vector<float> nco_table()
{
    // nco.proto.c: sintab[i] = sinf(2.0f*M_PI*(float)(i)/1024.0f)
    std::vector<float> t(1024);
    for (int i = 0; i < 1024; i++) t[i] = sinf((float)(2.0f * 3.14159265358979323846 * (float)i / 1024.0f));
    return t;
}

static uint32_t nco_constrain(float theta)
{
    const float p = (float)((double)theta * 0.159154943091895);
    float f = p - (float)(long long)p;
    if (f < 0.0f) f = (float)((double)f + 1.0);
    return (uint32_t)(long long)(f * 4294967296.0f);
}

// ====================================================================== IIR
struct IirObj : DevObj {
    bool cplx = true;
    bool sos = true;
    unsigned int nsos = 0;
    std::vector<float> b, a;          // SOS: [nsos][3] each; TF: nb, na (normalised by a0)
    int nb = 0, na = 0, nv = 0, D = 0;
    int mode = LDSP_MODE_FAST;
    int spec_W = 0;                   // > 0: fast-decaying filter -> speculative exact chunks
    DevBuf db, da, st32, st64, sc1, sc2, mats;
    DevBuf bmats, bsc1, bsc2, bsc3;   // blocked scan (D <= 8): matrices and scratch
    int bplan_G = 0;
    // single-pass modal scan (k_iir_modal.hip): the modal form (ok == false:
    // the blocked scan), its tables, the per-unit published end states, the
    // call epoch, and the modal state in two buffers (a call reads its start
    // state from mst and writes its end state into mstb; swapped after the call)
    ModalForm mf;
    DevBuf mtab, magg, mst, mstb;
    long magg_units = 0;
    uint32_t m_epoch = 0;
    int path_force = 0;               // ldsp_debug_iir_path: 0 auto, 1 blocked scan, 2 modal
    DevBuf iq;                        // int16 IQ converted for the paths that do not read it themselves
    DevBuf rsside, rsbuf;             // ldsp_iirfilt_resamp_execute: unit edges (fused) / filter output (two calls)
    enum { kSt32 = 0, kSt64 = 1, kStModal = 2 };
    int state_at = kSt32;             // where the authoritative state lives
    int plan_C = 0;
    long plan_nch = 0;
    int plan_G = 0;
    std::vector<double> A;            // D x D one-step state matrix (float64)

    int fsz() const { return sos ? 3 * (int)nsos : nv; }
    int ncomp() const { return cplx ? 2 : 1; }
    // Long look-backs: outside its one-XCD small-call mode (<= 16 J units) the
    // modal scan's 8 per-XCD unit ranges each start with J(J+1)/2 predecessor
    // recomputes (k_iir_modal.hip); a slowly decaying filter (J >= 16) whose
    // recomputes would exceed a quarter of the call's units takes the blocked scan.
    bool modal_pays(size_t n) const
    {
        const long units = k::iir_modal_units(n), J = mf.J;
        return J < 16 || units <= 16 * J || 4 * J * (J + 1) <= units / 4;
    }
    // which kernel path a call of n samples takes
    enum Path { kSpec, kSeq, kModal, kBlk, kScan };
    Path path_for(size_t n) const
    {
        // fast-decaying filters: speculative exact chunks (the sequential
        // loop's bits, so exact mode takes them too: FMStereo's de-emphasis)
        static const long spec_min = LDSP_KNOB("LDSP_IIR_SPEC_MIN", 0L);
        if (D == 0) return kSeq;
        if (path_force == 0 && spec_W > 0 && spec_W <= 16384 && (long)n >= spec_min) return kSpec;
        if (mode == LDSP_MODE_EXACT) return kSeq;
        if (mf.ok && path_force != 1 && (path_force >= 2 || modal_pays(n))) return kModal;
        return D <= k::kIirBlkMaxD ? kBlk : kScan;
    }

    // one step of the recursion on a state vector (the layout of the scan
    // kernels), in double or long double
    template <class R>
    R step_t(std::vector<R>& v, R x) const
    {
        if (sos) {
            R t = x;
            for (unsigned s = 0; s < nsos; s++) {
                const R v1 = v[2 * s], v2 = v[2 * s + 1];
                const R v0 = t - (R)a[3 * s + 1] * v1 - (R)a[3 * s + 2] * v2;
                t = (R)b[3 * s] * v0 + (R)b[3 * s + 1] * v1 + (R)b[3 * s + 2] * v2;
                v[2 * s + 1] = v1;
                v[2 * s] = v0;
            }
            return t;
        }
        R r = x;
        for (int i = 1; i < na; i++) r -= (R)a[i] * v[i - 1];
        R y = (R)b[0] * r;
        for (int i = 1; i < nb; i++) y += (R)b[i] * v[i - 1];
        for (int i = D - 1; i > 0; i--) v[i] = v[i - 1];
        if (D > 0) v[0] = r;
        return y;
    }
    double step_host(std::vector<double>& v, double x) const { return step_t<double>(v, x); }

    void finalize()
    {
        D = sos ? 2 * (int)nsos : nv - 1;
        A.assign((size_t)D * D, 0.0);
        for (int c = 0; c < D; c++) {
            std::vector<double> v(D, 0.0);
            v[c] = 1.0;
            step_host(v, 0.0);
            for (int r = 0; r < D; r++) A[(size_t)r * D + c] = v[r];
        }
        // modal form for the single-pass scan (long-double state space)
        mf = ModalForm{};
        if (D > 0) {
            using L = long double;
            std::vector<L> Al((size_t)D * D), Bl(D), Cl(D);
            for (int c = 0; c < D; c++) {
                std::vector<L> v(D, 0.0L);
                v[c] = 1.0L;
                Cl[c] = step_t<L>(v, 0.0L);
                for (int r = 0; r < D; r++) Al[(size_t)r * D + c] = v[r];
            }
            std::vector<L> v(D, 0.0L);
            const L Dd = step_t<L>(v, 1.0L);
            Bl = v;
            mf = modal_form(D, Al, Bl, Cl, Dd, sos ? sos_poles(a, nsos) : tf_poles(a, na, D));
        }
        // decay length: smallest 2^k with ||A^(2^k)||_inf < 2^-70
        spec_W = 0;
        if (D > 0) {
            std::vector<double> P = A;
            for (int k = 0; k <= 12; k++) {
                double nrm = 0;
                for (int r = 0; r < D; r++) {
                    double s = 0;
                    for (int q = 0; q < D; q++) s += fabs(P[(size_t)r * D + q]);
                    nrm = std::max(nrm, s);
                }
                if (nrm < 8.5e-22) {
                    spec_W = 2 << k;   // twice the decay length, as margin
                    break;
                }
                P = matmul(P, P);
            }
        }
    }
    std::vector<double> matmul(const std::vector<double>& X, const std::vector<double>& Y) const
    {
        std::vector<double> Z((size_t)D * D, 0.0);
        for (int r = 0; r < D; r++)
            for (int k = 0; k < D; k++) {
                const double x = X[(size_t)r * D + k];
                for (int c = 0; c < D; c++) Z[(size_t)r * D + c] += x * Y[(size_t)k * D + c];
            }
        return Z;
    }
    std::vector<double> matpow(std::vector<double> X, uint64_t e) const
    {
        std::vector<double> R((size_t)D * D, 0.0);
        for (int i = 0; i < D; i++) R[(size_t)i * D + i] = 1.0;
        while (e) {
            if (e & 1) R = matmul(R, X);
            X = matmul(X, X);
            e >>= 1;
        }
        return R;
    }
    void bind(int dev)
    {
        upload(db, b, dev);
        upload(da, a, dev);
        st32.ensure(sizeof(float) * 2 * std::max(fsz(), 1), dev);
        zero_now(st32.p, 0, sizeof(float) * 2 * std::max(fsz(), 1));
        st64.ensure(sizeof(double) * 2 * std::max(D, 1), dev);
        zero_now(st64.p, 0, sizeof(double) * 2 * std::max(D, 1));
        if (mf.ok) {
            const size_t mb = sizeof(double) * 2 * 2 * mf.M;
            zero_now(mst.ensure(mb, dev), 0, mb);
            mstb.ensure(mb, dev);
            upload(mtab, mf.tables, dev);
        }
        state_at = kSt32;
    }
    k::IirDesc desc() const
    {
        k::IirDesc d;
        d.sos = sos ? 1 : 0;
        d.nsos = (int)nsos;
        d.nb = nb;
        d.na = na;
        d.nv = nv;
        d.D = D;
        d.b = db.as<float>();
        d.a = da.as<float>();
        return d;
    }
    // Move the authoritative state between the float32 DF-II layout (exact
    // paths), the float64 layout of the SOS-coordinate scans and the modal
    // coordinates (k_iir_modal), through the host (mode switches only).
    void state_to(int to, hipStream_t s)
    {
        if (state_at == to) return;
        const int nc = ncomp(), fs = fsz();
        std::vector<double> d(2 * std::max(D, 1), 0.0);
        LDSP_HIP(hipStreamSynchronize(s));
        // 1. current state -> float64 layout d
        if (state_at == kSt32) {
            std::vector<float> f(2 * std::max(fs, 1), 0.0f);
            LDSP_HIP(hipMemcpy(f.data(), st32.p, f.size() * 4, hipMemcpyDeviceToHost));
            for (int c = 0; c < nc; c++) {
                if (sos)
                    for (unsigned q = 0; q < nsos; q++) {
                        d[c * D + 2 * q] = f[c * fs + 3 * q];
                        d[c * D + 2 * q + 1] = f[c * fs + 3 * q + 1];
                    }
                else
                    for (int i = 0; i < D; i++) d[c * D + i] = f[c * fs + i];
            }
        } else if (state_at == kSt64) {
            LDSP_HIP(hipMemcpy(d.data(), st64.p, d.size() * 8, hipMemcpyDeviceToHost));
        } else {
            const int M = mf.M;
            std::vector<double> v(2 * 2 * M);
            LDSP_HIP(hipMemcpy(v.data(), mst.p, v.size() * 8, hipMemcpyDeviceToHost));
            for (int c = 0; c < nc; c++)
                for (int i = 0; i < D; i++) {
                    double t = 0;
                    for (int q = 0; q < 2 * M; q++) t += mf.from_v[(size_t)i * 2 * M + q] * v[c * 2 * M + q];
                    d[c * D + i] = t;
                }
        }
        // 2. float64 layout -> target
        if (to == kSt32) {
            std::vector<float> f(2 * std::max(fs, 1), 0.0f);
            for (int c = 0; c < nc; c++) {
                if (sos)
                    for (unsigned q = 0; q < nsos; q++) {
                        f[c * fs + 3 * q] = (float)d[c * D + 2 * q];
                        f[c * fs + 3 * q + 1] = (float)d[c * D + 2 * q + 1];
                        f[c * fs + 3 * q + 2] = 0.0f;
                    }
                else
                    for (int i = 0; i < fs; i++) f[c * fs + i] = i < D ? (float)d[c * D + i] : 0.0f;
            }
            LDSP_HIP(hipMemcpy(st32.p, f.data(), f.size() * 4, hipMemcpyHostToDevice));
        } else if (to == kSt64) {
            LDSP_HIP(hipMemcpy(st64.p, d.data(), d.size() * 8, hipMemcpyHostToDevice));
        } else {
            const int M = mf.M;
            std::vector<double> v(2 * 2 * M, 0.0);
            for (int c = 0; c < nc; c++)
                for (int q = 0; q < 2 * M; q++) {
                    double t = 0;
                    for (int i = 0; i < D; i++) t += mf.to_v[(size_t)q * D + i] * d[c * D + i];
                    v[c * 2 * M + q] = t;
                }
            LDSP_HIP(hipMemcpy(mst.p, v.data(), v.size() * 8, hipMemcpyHostToDevice));
        }
        state_at = to;
    }
    // Blocked scan plan (k_iir_blk): 256-sample chunks, 256 chunks per block.
    k::IirBlkPlan blk_plan(size_t n)
    {
        const long C = k::kIirBlkChunk, CB = C * k::kIirBlkChunks;
        const long nch = (long)((n + C - 1) / C);
        const long nblk = (long)((n + CB - 1) / CB);
        const int G = (int)((nblk + 1023) / 1024);
        const size_t DD = (size_t)D * D;
        if (G != bplan_G) {
            std::vector<double> all;
            std::vector<double> M = matpow(A, (uint64_t)C);
            for (int l = 0; l < 8; l++) {                     // A^{C 2^l}
                all.insert(all.end(), M.begin(), M.end());
                M = matmul(M, M);
            }
            const std::vector<double> AB = matpow(A, (uint64_t)CB);
            all.insert(all.end(), AB.begin(), AB.end());
            M = matpow(AB, (uint64_t)G);
            for (int l = 0; l < 10; l++) {                    // A^{CB G 2^l}
                all.insert(all.end(), M.begin(), M.end());
                M = matmul(M, M);
            }
            upload(bmats, all, device);
            bplan_G = G;
        }
        k::IirBlkPlan p;
        p.nchunks = nch;
        p.nblk = nblk;
        p.G = G;
        p.AL = bmats.as<double>();
        p.AB = p.AL + 8 * DD;
        p.AG = p.AB + DD;
        p.local = (double*)bsc1.ensure((size_t)nch * ncomp() * D * sizeof(double), device);
        p.blocal = (double*)bsc2.ensure((size_t)nblk * ncomp() * D * sizeof(double), device);
        p.bstart = (double*)bsc3.ensure((size_t)nblk * ncomp() * D * sizeof(double), device);
        return p;
    }
    // one XCD while its 32 CUs stream the call faster than a range start
    // recomputes its J predecessors (~2.5 us each): up to 16 J units
    // (modal_plan, ldsp_debug_iir_modal_grid)
    int modal_one_xcd(size_t n) const
    {
        static const int onex = LDSP_KNOB("LDSP_IIR_ONEXCD", -1);
        return onex >= 0 ? onex : (k::iir_modal_units(n) <= 16L * mf.J ? 1 : 0);
    }
    // Modal scan plan: the tables (uploaded with the state), the per-unit
    // granules (zero when allocated: below every epoch) and this call's epoch.
    k::IirModalPlan modal_plan(size_t n)
    {
        const long units = k::iir_modal_units(n);
        const size_t per = (size_t)ncomp() * mf.M * 4 * sizeof(uint64_t);
        if (units > magg_units) {
            magg.ensure((size_t)units * per, device);
            zero_now(magg.p, 0, magg.cap);
            magg_units = (long)(magg.cap / per);
        }
        if (++m_epoch == 0) {                         // wrapped: restart the granules
            zero_now(magg.p, 0, magg.cap);
            m_epoch = 1;
        }
        k::IirModalPlan p;
        p.J = mf.J;
        p.PS = mtab.as<double>();
        p.PL = p.PS + 6 * mf.M * 4;
        p.PB = p.PL + 64 * mf.M * 4;
        p.agg = magg.as<uint64_t>();
        p.epoch = m_epoch;
        p.recompute = path_force == 3 ? 1 : 0;
        p.one_xcd = modal_one_xcd(n);
        p.variant = LDSP_KNOB("LDSP_IIR_VARIANT", 0);
        return p;
    }
    // Speculative exact chunks (kSpec): warm-up, chunk length and count; the
    // caller adds the scratch.
    k::SpecPlan spec_plan(size_t n) const
    {
        k::SpecPlan p;
        p.W = spec_W;
        p.C = std::max(128, spec_W / 32);   // W + C steps per lane, <= 1/32 redundancy growth
        p.nchunks = (long)((n + p.C - 1) / p.C);
        p.scratch = nullptr;
        return p;
    }
    k::IirScanPlan scan_plan(size_t n)
    {
        int C = 64;
        while (C < 1024 && (size_t)C * 65536 < n) C <<= 1;
        const long nch = (long)((n + C - 1) / C);
        const int G = (int)((nch + 1023) / 1024);
        if (C != plan_C || G != plan_G) {
            const std::vector<double> AC = matpow(A, (uint64_t)C);
            std::vector<double> M = matpow(AC, (uint64_t)G);
            std::vector<double> all(AC);
            for (int l = 0; l < 10; l++) {
                all.insert(all.end(), M.begin(), M.end());
                M = matmul(M, M);
            }
            upload(mats, all, device);
            plan_C = C;
            plan_G = G;
        }
        plan_nch = nch;
        const size_t need = (size_t)nch * ncomp() * D * sizeof(double);
        sc1.ensure(need, device);
        sc2.ensure(need, device);
        k::IirScanPlan p;
        p.C = C;
        p.nchunks = nch;
        p.G = G;
        p.levels = 10;
        p.AC = mats.as<double>();
        p.AG = mats.as<double>() + (size_t)D * D;
        p.local = sc1.as<double>();
        p.carry = sc2.as<double>();
        return p;
    }
};

// ====================================================================== AGC
struct AgcObj : DevObj {
    k::AgcState h{};                  // host mirror
    float bandwidth = 0.01f;
    DevBuf dst, status;
    // Per-call scratch in two slots (call parity) and the input history the
    // speculative warm-ups read (the last hist_len samples before the call, in
    // a ring of three: call k reads hist[k % 3] and writes hist[(k + 1) % 3], so
    // call k + 1's front may start while call k's chunks still read theirs;
    // call k + 2, which overwrites it, first waits for call k's back half).
    DevBuf scr[2], hist[3];
    long hist_len = 0, hist_valid = 0;
    uint64_t ncall = 0;
    bool dev_newer = false;           // device state advanced past the mirror
    bool upload_pending = true;
    // Cross-stream order (ldsp_common.hpp): ord = back halves (the true
    // state), front = front halves (history), slot[s] = scratch slot s free.
    StreamMark front, slot[2];
    int tsa_perturb = 0;              // ldsp_debug_agc_tsa_perturb (test hook)
    int perturb = 0;                  // ldsp_debug_agc_perturb (test hook, chunk-parallel calls)
    int rounds_force = -1;            // ldsp_debug_agc_rounds (test hook; -1: the default)
    void init()
    {
        // agc_crcf_create: bandwidth 0.01, reset (g=1, y2'=1), squelch disabled,
        // threshold 0, timeout 100, scale 1
        bandwidth = 0.01f;
        h.alpha = bandwidth;
        h.g = 1.0f;
        h.y2p = 1.0f;
        h.locked = 0;
        h.mode = 7;
        h.threshold = 0.0f;
        h.timeout = 100;
        h.timer = 0;
        h.scale = 1.0f;
    }
    void pull()
    {
        if (!dev_newer) return;
        LDSP_HIP(hipStreamSynchronize(last));
        DeviceGuard g(device);
        LDSP_HIP(hipMemcpy(&h, dst.p, sizeof(h), hipMemcpyDeviceToHost));
        dev_newer = false;
    }
    void modified() { upload_pending = true; }
    void bind(int dev)
    {
        dst.ensure(sizeof(k::AgcState), dev);
        upload_pending = true;
    }
};

// ====================================================================== AmpModem
// Live PLL objects (AmpModem, BroadcastAM) per device: a walker may be launched
// before its predecessor has finished (amp_pll_stage), holding a CU while it
// waits.  Waiting walkers and the walkers they wait for number at most twice the
// live objects on the device, so the early path is taken only while those stay
// within half the device's CUs (amp_early_max: CUs / 4 objects, 64 on MI355X; a
// CPX-partitioned device gets its own, smaller bound).  Other processes sharing
// the GPU are not counted: their walkers can only delay a hand-off, which the
// walker's bounded wait turns into LDSP_EHIP at the next call (amp_check_err),
// never into a silent result.
static constexpr int kAmpMaxDev = 64;
static std::atomic<int> g_amp_live[kAmpMaxDev];
static int amp_early_max(int dev)
{
    static std::atomic<int> cache[kAmpMaxDev];
    if (dev < 0 || dev >= kAmpMaxDev) return 0;
    int v = cache[dev].load();
    if (v == 0) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 0;
        v = cus / 4 > 0 ? cus / 4 : -1;
        cache[dev] = v;
    }
    return v;
}
struct AmpLive {
    int dev = -1;
    void set(int d)
    {
        if (dev < 0 && d >= 0 && d < kAmpMaxDev) {
            dev = d;
            g_amp_live[d]++;
        }
    }
    bool early_ok() const { return dev >= 0 && g_amp_live[dev].load() <= amp_early_max(dev); }
    AmpLive() = default;
    ~AmpLive()
    {
        if (dev >= 0) g_amp_live[dev]--;
    }
    AmpLive(const AmpLive&) = delete;
    AmpLive& operator=(const AmpLive&) = delete;
};
// Host-mapped error flags (one word per PLL object, taken from page-sized
// blocks that are never freed: hipHostFree at teardown can outlive the runtime).
// A walker whose hand-off wait times out sets its object's flag; every call
// checks it on entry (amp_check_err), so a bad walk is reported at the latest by
// the object's next call even when no call synchronises in between.
struct ErrFlags {
    std::mutex mu;
    std::vector<uint32_t*> free_list;
    uint32_t* take()
    {
        std::lock_guard<std::mutex> lk(mu);
        if (free_list.empty()) {
            void* p = nullptr;
            LDSP_HIP(hipHostMalloc(&p, 4096, hipHostMallocMapped | hipHostMallocCoherent));
            for (int i = 1023; i >= 0; i--) free_list.push_back((uint32_t*)p + i);
        }
        uint32_t* f = free_list.back();
        free_list.pop_back();
        *(volatile uint32_t*)f = 0;
        return f;
    }
    void give(uint32_t* f)
    {
        std::lock_guard<std::mutex> lk(mu);
        free_list.push_back(f);
    }
};
static ErrFlags& err_flags()
{
    static ErrFlags* e = new ErrFlags();   // never destroyed (see above)
    return *e;
}
static constexpr unsigned long long kWalkWaitTicks = 100000000ull;   // 1 s of s_memrealtime (100 MHz)
// ldsp_debug_walk_early: -1 default (early hand-off on), 0 / 1 forced
static std::atomic<int> g_walk_early{-1};
struct AmpObj : DevObj {
    AmpLive live;
    uint32_t* herr = nullptr;             // host-mapped walker timeout flag (ErrFlags)
    float mod_index = 0.75f;
    int type = 0;
    int suppressed = 1;
    unsigned int m = 25;
    std::vector<float> lp, dc, hq, table;     // hq: the usb / lsb Hilbert transform's 2m quadrature taps
    k::AmpState st{};
    DevBuf dlp, ddc, dtab, dst;
    PingPong lph, dch;                        // carrier lowpass and DC blocker histories (flipped together)
    // usb / lsb: Hilbert taps, its input history (4m - 1 samples, ping-pong) and per-slot v1 scratch
    DevBuf dhq, v1[2];
    PingPong hbh;
    // Per-call scratch in two slots (call parity) and the delay-line history in
    // three (call index mod 3), so that call k's front half (lowpass, history,
    // candidates) can run while call k-1's walker still reads its own slot.
    DevBuf x0[2], mb[2], pll[2], dlh[3];
    unsigned long long ncall = 0;
    uint32_t wexp = 0;                    // launches issued that write the PLL state (AmpState::wepoch)
    size_t last_pll_n = 0;                // samples of the last call's PLL launch
    const void* last_stats = nullptr;     // walker counters of the last parallel call (in its scratch slot)
    bool dev_newer = false;
    // Cross-stream order (ldsp_common.hpp): `front` = end of a call's front half
    // (lowpass + delay histories, candidate guess state), `ord` = end of a call's
    // walk (true PLL state), `post` = end of its DC blocker (history),
    // `slot[i]` = end of the last call that used scratch slot i.
    StreamMark front, post, slot[2];
    void reset_host()
    {
        st.theta = 0;
        st.dtheta = 0;
        st.alpha = 0.001f;
        st.beta = sqrtf(st.alpha);
        for (int i = 0; i < 2; i++) {
            st.gth[i] = st.theta;
            st.gd[i] = st.dtheta;
        }
    }
    void sync_all()
    {
        ord.sync();
        post.sync();
        front.sync();
        for (auto& sm : slot) sm.sync();
    }
    void bind(int dev)
    {
        std::vector<float> lr(lp.rbegin(), lp.rend()), dr(dc.rbegin(), dc.rend());
        upload(dlp, lr, dev);
        upload(ddc, dr, dev);
        upload(dtab, table, dev);
        dst.ensure(sizeof(k::AmpState), dev);
        st.wepoch = wexp;
        if (!herr) herr = err_flags().take();
        void* hdev = nullptr;
        LDSP_HIP(hipHostGetDevicePointer(&hdev, herr, 0));
        st.herr = (uint32_t*)hdev;
        if (!st.wait_ticks) st.wait_ticks = kWalkWaitTicks;
        LDSP_HIP(hipMemcpy(dst.p, &st, sizeof(st), hipMemcpyHostToDevice));
        live.set(dev);
        lph.zero((2 * m) * 8, dev);
        dch.zero((2 * m) * 4, dev);
        for (auto& b : dlh) zero_now(b.ensure(m * 8, dev), 0, m * 8);
        if (!hq.empty()) {
            upload(dhq, hq, dev);
            hbh.zero((4 * m - 1) * 8, dev);
        }
    }
    AmpObj() = default;
    AmpObj(const AmpObj&) = delete;
    AmpObj& operator=(const AmpObj&) = delete;
    ~AmpObj()
    {
        if (herr) err_flags().give(herr);
    }
};

} // namespace ldsp

struct ldsp_resamp_s : ldsp::ResampObj {};
struct ldsp_nco_s : ldsp::NcoObj {};
struct ldsp_iirfilt_s : ldsp::IirObj {};
struct ldsp_agc_s : ldsp::AgcObj {};
struct ldsp_ampmodem_s : ldsp::AmpObj {};

// BroadcastAM: the AmpModem carrier-PLL stage with mod_index 1 (re(v1) / 1
// == re(v1)) followed by an owned SOS IIR DC blocker instead of the FIR one.
struct ldsp_bcastam_s : ldsp::AmpObj {
    ldsp_iirfilt_t dcb = nullptr;
    ~ldsp_bcastam_s() { ldsp_iirfilt_destroy(dcb); }
};

struct ldsp_freqdem_s : ldsp::DevObj {
    float kf = 0.0f, ref = 0.0f;
    ldsp::PingPong prev;                    // the last input sample
    void bind(int dev) { prev.zero(8, dev); }
};

// FMStereo (demod.hpp:4-85): freqdem(4) + mixer loop + two TF de-emphasis
// filters (exact) + two resamp_rrrf_create_default resamplers.
struct ldsp_fmstereo_s : ldsp::DevObj {
    float iq_rate = 0, pcm_rate = 0;
    ldsp_freqdem_t dem = nullptr;
    ldsp_iirfilt_t emph[2] = {nullptr, nullptr};
    ldsp_resamp_t aud[2] = {nullptr, nullptr};
    std::vector<float> table;
    ldsp::k::FmState st{};
    ldsp::DevBuf dst, dtab, sbuf, lr[2], le[2], out[2];
    void bind(int dev)
    {
        dst.ensure(sizeof(st), dev);
        LDSP_HIP(hipMemcpy(dst.p, &st, sizeof(st), hipMemcpyHostToDevice));
        ldsp::upload(dtab, table, dev);
    }
    ~ldsp_fmstereo_s()
    {
        ldsp_freqdem_destroy(dem);
        for (int c = 0; c < 2; c++) {
            ldsp_iirfilt_destroy(emph[c]);
            ldsp_resamp_destroy(aud[c]);
        }
    }
};

struct ldsp_delay_s : ldsp::DevObj {
    unsigned int nd = 1;
    ldsp::PingPong hr, hc;         // real / complex lines of nd + 1 samples
    void zero(int dev)
    {
        hr.zero((nd + 1) * 4, dev);
        hc.zero((nd + 1) * 8, dev);
    }
    void bind(int dev) { zero(dev); }
};

// firhilbf (SSBDemod, HilbertTransform): the 2m quadrature taps and, on the
// device, the last H input samples in the input's layout, ping-ponged.
struct ldsp_firhilb_s : ldsp::DevObj {
    unsigned int m = 0;
    int op = 0;
    std::vector<float> hq;
    ldsp::DevBuf dhq;
    ldsp::PingPong hist;
    ldsp::Staging stg1;                    // the second output of a host-memory C2R call
    size_t in_size() const { return op == LDSP_HILB_C2R || op == LDSP_HILB_INTERP ? 8 : 4; }
    size_t hist_bytes() const { return (size_t)(op == LDSP_HILB_INTERP ? 2 * m - 1 : 4 * m - 1) * in_size(); }
    void bind(int dev)
    {
        std::vector<float> pad(hq);
        pad.resize(pad.size() + ldsp::k::kHilbTapPad, 0.0f);
        ldsp::upload(dhq, pad, dev);
        hist.zero(hist_bytes(), dev);
    }
};

// Where a decimating T stands in its stream (T::D, T::seen): the samples before the next output, the outputs of n samples
template <class T>
struct Decimating {
    const T& self() const { return static_cast<const T&>(*this); }
    size_t skip() const { return (size_t)((self().D - self().seen % self().D) % self().D); }
    size_t num_outputs(size_t n) const { return n > skip() ? (n - skip() + self().D - 1) / self().D : 0; }
};

// The two polyphase banks: the prototype, the host-side stream position, and
// on the device the taps padded to kChanMaxP M, the twiddle table
// exp(2 pi i j / M), j < M, as (re, im) pairs (double, rounded once) and the
// input history, ping-ponged.
struct BankObj : ldsp::DevObj {
    unsigned int M = 0, D = 0;
    unsigned int R = 0;                    // taps per branch: the Channelizer's P, the Synthesizer's Q
    std::vector<float> h;
    float scale = 1.0f;
    uint64_t seen = 0;                     // input samples (Synthesizer: columns) since create / reset
    size_t hist_bytes = 0;
    ldsp::DevBuf dtaps, dtw;
    ldsp::PingPong hist;
    void bind(int dev)
    {
        std::vector<float> pad(h);
        pad.resize((size_t)ldsp::k::kChanMaxP * M, 0.0f);
        ldsp::upload(dtaps, pad, dev);
        std::vector<float> tw(2 * (size_t)M);
        for (unsigned j = 0; j < M; j++) {
            const double a = 2.0 * M_PI * (double)j / (double)M;
            tw[2 * j] = (float)cos(a);
            tw[2 * j + 1] = (float)sin(a);
        }
        ldsp::upload(dtw, tw, dev);
        hist.zero(hist_bytes, dev);
    }
};

// Channelizer (polyphase analysis bank): skip and the output parity follow from
// the samples seen; the history is the last P M - 1 input samples.
struct ldsp_chan_s : BankObj, Decimating<ldsp_chan_s> {
    int parity() const { return (int)(((seen + D - 1) / D) & 1); }   // of the next output's absolute index
};

// Synthesizer (polyphase synthesis bank): the D = M / 2 sign's parity follows
// from the columns seen; the history is the last Q - 1 input columns as [M][Q - 1].
struct ldsp_synth_s : BankObj {};

// Downconverter (tuned decimating bank): the prototype, the frequency words,
// the host-side stream position (skip and the first column's absolute index
// follow from it), and on the device the complex taps g_c in the kernel's
// layout (kernels.hpp), the words and the last L - 1 raw input samples,
// ping-ponged.  The history is raw input, so a retune touches the tables alone.
struct ldsp_ddc_s : ldsp::DevObj, Decimating<ldsp_ddc_s> {
    unsigned int D = 0;
    std::vector<float> h;
    std::vector<uint32_t> w;
    float scale = 1.0f;
    uint64_t seen = 0;                     // input samples since create / reset (or the seek hook's T)
    ldsp::DevBuf dtaps, dwords, dslots;
    ldsp::PingPong hist;
    size_t hist_bytes() const { return std::max<size_t>(h.size() - 1, 1) * 8; }
    uint64_t next_column() const { return seen / D + (seen % D != 0); }
    // g_c[j] = h[j] exp(+2 pi i ((j w_c) mod 2^32) / 2^32) in double, rounded once, as
    // [tuner block][k = L - 1 - j][TB]; the phase as a signed count of 2^-31 half-turns
    void upload_tables(int dev)
    {
        const size_t C = w.size(), L = h.size();
        const size_t TB = (size_t)ldsp::k::ddc_block((int)C), nb = (C + TB - 1) / TB;
        std::vector<float> g(2 * nb * L * TB, 0.0f);
        for (size_t c = 0; c < C; c++)
            for (size_t j = 0; j < L; j++) {
                const uint32_t ph = (uint32_t)j * w[c];
                const double a = M_PI * ((double)(int32_t)ph / 2147483648.0);
                const size_t at = ((c / TB * L + (L - 1 - j)) * TB + c % TB) * 2;
                g[at] = (float)((double)h[j] * cos(a));
                g[at + 1] = (float)((double)h[j] * sin(a));
            }
        ldsp::upload(dtaps, g, dev);
        std::vector<uint32_t> wp(w);
        wp.resize(nb * TB, 0u);
        ldsp::upload(dwords, wp, dev);
    }
    void bind(int dev)
    {
        upload_tables(dev);
        std::vector<int> slots(h.size());
        for (size_t k = 0; k < slots.size(); k++) slots[k] = ldsp::k::ddc_slot((int)D, (int)h.size(), (int)k);
        ldsp::upload(dslots, slots, dev);
        hist.zero(hist_bytes(), dev);
    }
};

// FMBank (discriminator and decimating FIR over bank rows): the prototype (none:
// the discriminator alone, D = 1), the host-side stream position (skip follows
// from it), and on the device the taps in the kernel's layout (kernels.hpp),
// per row the last L - 1 discriminator values and the last raw sample, both
// ping-ponged.  The history holds discriminator values, so zeroed buffers are
// the definition's "d = 0 before t = 0".
struct ldsp_fmbank_s : ldsp::DevObj, Decimating<ldsp_fmbank_s> {
    unsigned int C = 0, D = 1;
    float ref = 0.0f;                      // (float)(1 / (2 pi kf))
    std::vector<float> h;                  // empty: the discriminator alone
    float scale = 1.0f;
    uint64_t seen = 0;                     // input samples per row since create / reset
    ldsp::DevBuf dtaps;
    ldsp::PingPong dhist, prev;
    size_t hist_bytes() const { return std::max<size_t>((size_t)C * (h.empty() ? 0 : h.size() - 1), 1) * 4; }
    void zero_state(int dev)
    {
        dhist.zero(hist_bytes(), dev);
        prev.zero((size_t)C * 8, dev);
    }
    void bind(int dev)
    {
        // t[r][q] = h[L - 1 - (q D + r)], zero past the prototype's end
        const size_t L = h.size(), QP = (L + D - 1) / D;
        std::vector<float> t((size_t)D * QP, 0.0f);
        for (size_t k = 0; k < L; k++) t[(k % D) * QP + k / D] = h[L - 1 - k];
        ldsp::upload(dtaps, t, dev);
        zero_state(dev);
    }
};

// AudioBank (de-emphasis and polyphase resampler over bank rows): the resampler's
// design and its host-side phase (as ResampObj's), the de-emphasis coefficients
// and warm-up (J = 0: none), the samples per row since reset (the de-emphasis
// grid is absolute), and on the device the branch table in the kernel's layout
// and per row the last H raw input samples, ping-ponged.
struct ldsp_audiobank_s : ldsp::DevObj {
    unsigned int C = 0, m = 0, npfb = 0, sub_len = 0;
    int bits_index = 0;
    float rate = 1.0f;
    uint32_t step = 0;
    uint64_t phase = 0, seen = 0;
    std::vector<float> hproto, sub;        // sub: [npfb][sub_len] reversed
    float sample_rate = 0.0f;              // <= 0: no de-emphasis
    double tau = 0.0;
    float a = 0.0f, b0 = 1.0f;
    int J = 0, H = 0;
    bool pcm16 = false;
    float scale = 1.0f;
    ldsp::DevBuf dsub;
    ldsp::PingPong hist;
    size_t hist_bytes() const { return (size_t)C * H * 4; }
    size_t osz() const { return pcm16 ? 2 : 4; }
    size_t num_outputs(size_t n) const     // ResampObj::num_outputs
    {
        if (n == 0) return 0;
        const long long num = (long long)(n - 1) * (1LL << 24) + 0xffffffLL - (long long)phase;
        return num < 0 ? 0 : (size_t)(num / step) + 1;
    }
    int tile() const { return ldsp::k::audiobank_tile(step, (int)sub_len, (int)npfb, J); }
    void bind(int dev)
    {
        std::vector<float> t((size_t)npfb * (sub_len + 1), 0.0f);   // rows padded to an odd length
        for (size_t b = 0; b < npfb; b++) std::copy_n(&sub[b * sub_len], sub_len, &t[b * (sub_len + 1)]);
        ldsp::upload(dsub, t, dev);
        hist.zero(hist_bytes(), dev);
    }
};

// SquelchBank (per-row level and squelch gate over bank rows): the thresholds
// in dB as set and as the float32 the kernel compares, the host-side stream
// position (fill and the block count of a call follow from it), and on the
// device the thresholds, per row the smoothed power, mode and timer (updated in
// place by the one lane that owns the row), the carried samples of the
// unfinished block as [C][B], ping-ponged, and the block powers of one call.
struct ldsp_sqbank_s : ldsp::DevObj {
    unsigned int C = 0, B = 0, timeout = 0;
    double alpha = 0.0;
    std::vector<double> thr_db;
    std::vector<float> thr;
    uint64_t seen = 0;                     // input samples per row since create / reset
    ldsp::DevBuf dthr, dstate, dpow;
    ldsp::PingPong hist;
    ldsp::Staging stg_status, stg_level;   // the other two outputs of a host-memory call (stg: x and y)
    size_t fill() const { return (size_t)(seen % B); }
    size_t num_outputs(size_t K) const { return (size_t)((seen + K) / B - seen / B); }
    static ldsp::k::SqState initial() { return {0.0, 1, 0}; }   // s = 0, ENABLED, timer 0
    void zero_state(int dev)
    {
        ldsp::upload(dstate, std::vector<ldsp::k::SqState>(C, initial()), dev);
        hist.zero((size_t)C * B * 8, dev);
    }
    void bind(int dev)
    {
        ldsp::upload(dthr, thr, dev);
        zero_state(dev);
    }
};

// AGCBank (look-ahead hang AGC over bank rows): the parameters in dB as given and
// in the tracker's integer units, the host-side stream position (the blocks
// tracked and emitted, the carried samples and the pending block follow from
// it), and on the device the targets, per row the tracker level, the last H
// peaks, the two boundary gains in flight, the samples not yet emitted as
// [C][2B], ping-ponged, and the gains of one call.
struct ldsp_agcbank_s : ldsp::DevObj {
    unsigned int C = 0, B = 0, H = 0;
    bool cplx = false;
    double max_gain_db = 0.0, decay_db = 0.0;
    std::vector<double> target_db;
    std::vector<int32_t> T;
    int32_t Gmax = 0;
    int64_t d = 0;
    uint64_t seen = 0;                     // input samples per row since create / reset
    ldsp::DevBuf dtarget, dlevel, dtail, dedge, dgains;
    ldsp::PingPong hist;
    ldsp::Staging stg_peak, stg_gain;      // the other two outputs of a host-memory call (stg: x and y)
    size_t esz() const { return cplx ? 8 : 4; }
    uint64_t tracked(uint64_t s) const { return s / B; }
    uint64_t emitted(uint64_t s) const { return s / B > 0 ? s / B - 1 : 0; }
    size_t fill() const { return (size_t)(seen - emitted(seen) * B); }
    int pend() const { return seen >= B ? 1 : 0; }
    void zero_state(int dev)
    {
        ldsp::upload(dlevel, std::vector<int32_t>(C, ldsp::agc::kAgcFloor), dev);
        ldsp::upload(dtail, std::vector<int32_t>((size_t)C * ldsp::k::kAgcbankTail, ldsp::agc::kAgcFloor), dev);
        ldsp::upload(dedge, std::vector<float>((size_t)C * 2, 0.0f), dev);
        hist.zero((size_t)C * 2 * B * esz(), dev);
    }
    void bind(int dev)
    {
        ldsp::upload(dtarget, T, dev);
        zero_state(dev);
    }
};

// ToneBank (per-row tone detector and tone squelch over bank rows): the tones and
// the two tables as handed back, the settings, the host-side stream position
// (fill and the block count of a call follow from it), and on the device the
// tables in the power kernel's layout, the wanted tone per row, per row the
// blocks since the last accepted one and the carried samples of the unfinished
// block as [C][B], both ping-ponged, and the open flags of a call that passes none.
struct ldsp_tonebank_s : ldsp::DevObj {
    unsigned int C = 0, F = 0, B = 0, hold = 0;
    int window = 0;
    double dominance = 0.0, sumw = 0.0;
    float floor = 0.0f;
    std::vector<double> tones;
    std::vector<float> tc, ts;             // [F][B] each
    std::vector<int8_t> want;
    uint64_t seen = 0;                     // input samples per row since create / reset
    ldsp::DevBuf dtab, dwant, dopen;
    ldsp::PingPong hist, since;
    ldsp::Staging stg_power, stg_tone, stg_open;   // the other outputs of a host-memory call (stg: x and y)
    size_t fill() const { return (size_t)(seen % B); }
    size_t num_outputs(size_t K) const { return (size_t)((seen + K) / B - seen / B); }
    void zero_state(int dev)
    {
        hist.zero((size_t)C * B * 4, dev);
        const std::vector<int> none(C, ldsp::k::kTonebankSat);
        for (auto& d : since.b) ldsp::upload(d, none, dev);
        since.cur = 0;
    }
    void bind(int dev)
    {
        std::vector<float> t;
        ldsp::k::tonebank_pack((int)F, (int)B, tc.data(), ts.data(), t);
        ldsp::upload(dtab, t, dev);
        ldsp::upload(dwant, want, dev);
        zero_state(dev);
    }
};

// StereoBank (FM stereo decoder over bank rows): the two prototypes, the pilot
// word and threshold, the host-side stream position (skip follows from it), and
// on the device the tap table in the kernel's layout (kernels.hpp), per row the
// last L - 1 raw samples, ping-ponged, and per row the pilot level of the last
// column emitted.  The history is raw input, so a new threshold touches no state.
struct ldsp_stbank_s : ldsp::DevObj, Decimating<ldsp_stbank_s> {
    unsigned int C = 0, D = 1;
    uint32_t w = 0;
    float thr = 0.0f;
    std::vector<float> h, g;               // audio and pilot prototypes, the same length
    uint64_t seen = 0;                     // input samples per row since create / reset
    ldsp::DevBuf dtaps, dlevel;
    ldsp::PingPong hist;
    size_t hist_bytes() const { return std::max<size_t>((size_t)C * (h.size() - 1), 1) * 4; }
    void zero_state(int dev)
    {
        hist.zero(hist_bytes(), dev);
        ldsp::zero_now(dlevel.ensure((size_t)C * 4, dev), 0, (size_t)C * 4);
    }
    // gz[j] = h[j] exp(+2 pi i ((j 2w) mod 2^32) / 2^32), gp[j] = g[j] exp(+2 pi i ((j w) mod 2^32) / 2^32)
    // in double, rounded once; the phase as a signed count of 2^-31 half-turns
    void bind(int dev)
    {
        const size_t L = h.size();
        std::vector<float> t(8 * L, 0.0f);
        for (size_t j = 0; j < L; j++) {
            const double az = M_PI * ((double)(int32_t)((uint32_t)j * (2u * w)) / 2147483648.0);
            const double ap = M_PI * ((double)(int32_t)((uint32_t)j * w) / 2147483648.0);
            float* e = &t[8 * (L - 1 - j)];
            e[0] = h[j];
            e[1] = (float)((double)h[j] * cos(az));
            e[2] = (float)((double)h[j] * sin(az));
            e[3] = (float)((double)g[j] * cos(ap));
            e[4] = (float)((double)g[j] * sin(ap));
            const int slot = ldsp::k::stbank_slot((int)D, (int)L, (int)(L - 1 - j));
            std::memcpy(&e[5], &slot, 4);
        }
        ldsp::upload(dtaps, t, dev);
        zero_state(dev);
    }
};

// AMBank (coherent AM demodulator over bank rows): the audio and the carrier
// prototype and their difference d, the threshold, the host-side stream position
// (skip follows from it), and on the device the tap table in the kernel's layout
// (kernels.hpp), per row the last L - 1 raw complex samples, ping-ponged, and
// per row the carrier level of the last column emitted.  The history is raw
// input, so a new threshold touches no state.
struct ldsp_ambank_s : ldsp::DevObj, Decimating<ldsp_ambank_s> {
    unsigned int C = 0, D = 1;
    float thr = 0.0f;
    std::vector<float> h, g, d;            // audio and carrier prototypes, the same length; d = h - g, rounded once
    uint64_t seen = 0;                     // input samples per row since create / reset
    ldsp::DevBuf dtaps, dlevel;
    ldsp::PingPong hist;
    size_t hist_bytes() const { return std::max<size_t>((size_t)C * (h.size() - 1), 1) * 8; }
    void zero_state(int dev)
    {
        hist.zero(hist_bytes(), dev);
        ldsp::zero_now(dlevel.ensure((size_t)C * 4, dev), 0, (size_t)C * 4);
    }
    void bind(int dev)
    {
        const size_t L = h.size();
        std::vector<float> t(4 * L, 0.0f);
        for (size_t j = 0; j < L; j++) {
            float* e = &t[4 * (L - 1 - j)];
            e[0] = d[j];
            e[1] = g[j];
            const int slot = ldsp::k::ambank_slot((int)D, (int)L, (int)(L - 1 - j));
            std::memcpy(&e[2], &slot, 4);
        }
        ldsp::upload(dtaps, t, dev);
        zero_state(dev);
    }
};

// SSBBank (tuned single-sideband demodulator over bank rows): the prototype, the
// band, per row the BFO, its word and the sideband, the complex taps g that
// follow from them (ldsp.h), the host-side stream position (skip and the first
// column's absolute index follow from it), and on the device the tap table in
// the kernel's layout (kernels.hpp), the words and per row the last L - 1 raw
// complex samples, ping-ponged.  The history is raw input, so a retune touches
// the tables alone.
struct ldsp_ssbbank_s : ldsp::DevObj, Decimating<ldsp_ssbbank_s> {
    unsigned int C = 0, D = 1;
    double lo = 0.0, hi = 0.0;
    std::vector<float> p;                  // the real low-pass prototype
    std::vector<double> bfo;               // as given, C entries
    std::vector<uint32_t> w;               // rint(bfo 2^32) mod 2^32
    std::vector<int> side;                 // +1 usb, -1 lsb
    std::vector<float> g;                  // [C][L] (re, im), index j
    uint64_t seen = 0;                     // input samples per row since create / reset (or the seek hook's T)
    ldsp::DevBuf dtaps, dwords;
    ldsp::PingPong hist;
    size_t hist_bytes() const { return std::max<size_t>((size_t)C * (p.size() - 1), 1) * 8; }
    uint64_t next_column() const { return seen / D + (seen % D != 0); }
    // psi_c[j] = (s_c wm (2j - (L - 1)) + 2 j w_c) mod 2^33 in integers, counts of 2^-33 turn;
    // g_c[j] = p[j] exp(2 pi i psi / 2^33) in double, the phase as a signed count, rounded once
    void make_taps()
    {
        const size_t L = p.size();
        const int64_t wm = (int64_t)std::nearbyint((lo + hi) * 0.5 * 4294967296.0);
        const int64_t M = (int64_t)1 << 33;
        g.assign(2 * (size_t)C * L, 0.0f);
        for (size_t c = 0; c < C; c++)
            for (size_t j = 0; j < L; j++) {
                int64_t psi = ((int64_t)side[c] * wm * (2 * (int64_t)j - (int64_t)(L - 1)) + 2 * (int64_t)j * (int64_t)w[c]) % M;
                if (psi < 0) psi += M;
                if (psi >= M / 2) psi -= M;           // [-2^32, 2^32): exact in double
                const double a = M_PI * ((double)psi / 4294967296.0);
                g[2 * (c * L + j)] = (float)((double)p[j] * cos(a));
                g[2 * (c * L + j) + 1] = (float)((double)p[j] * sin(a));
            }
    }
    void upload_tables(int dev)
    {
        const size_t L = p.size();
        std::vector<float> t(4 * (size_t)C * L, 0.0f);
        for (size_t c = 0; c < C; c++)
            for (size_t j = 0; j < L; j++) {
                float* e = &t[4 * (c * L + (L - 1 - j))];
                e[0] = g[2 * (c * L + j)];
                e[1] = g[2 * (c * L + j) + 1];
                const int slot = ldsp::k::ssbbank_slot((int)D, (int)L, (int)(L - 1 - j));
                std::memcpy(&e[2], &slot, 4);
            }
        ldsp::upload(dtaps, t, dev);
        ldsp::upload(dwords, w, dev);
    }
    void bind(int dev)
    {
        upload_tables(dev);
        hist.zero(hist_bytes(), dev);
    }
};

// Spectrogram (streaming Welch periodogram): the window, the host-side counts
// (samples since reset, transforms since clear; the schedule follows from
// them), and on the device the padded window, the twiddle table, the last
// W - 1 input samples and the unfinished row's sum (both ping-ponged), the
// float64 accumulator and the per-workgroup sums it is fed from.
struct ldsp_spgram_s : ldsp::DevObj {
    unsigned int N = 0, W = 0, d = 0, A = 0;
    std::vector<float> w;
    uint64_t seen = 0;                     // input samples since create / reset
    uint64_t nacc = 0;                     // transforms since create / reset / clear
    // carry: the unfinished row's sum (blocked averages: the unfinished block's);
    // blk, rcarry: a blocked average's block sums and its unfinished row's
    ldsp::DevBuf dwin, dtw, dpsd, part, blk;
    ldsp::PingPong hist, carry, rcarry;
    size_t hist_bytes() const { return std::max<size_t>((size_t)W - 1, 1) * 8; }
    size_t transforms(size_t n) const { return (size_t)((seen + n) / d - seen / d); }
    size_t rows(size_t n) const { return (size_t)((seen + n) / d / A - seen / d / A); }
    void zero_stream(int dev)
    {
        hist.zero(hist_bytes(), dev);
        carry.zero((size_t)N * 4, dev);
        rcarry.zero((size_t)N * 4, dev);
    }
    void zero_psd(int dev) { ldsp::zero_now(dpsd.ensure((size_t)N * 8, dev), 0, (size_t)N * 8); }
    void bind(int dev)
    {
        std::vector<float> pad(w);
        pad.resize(N, 0.0f);
        ldsp::upload(dwin, pad, dev);
        std::vector<float> tw(2 * (size_t)N);             // exp(-2 pi i j / N): double, rounded once
        for (unsigned j = 0; j < N; j++) {
            const double a = -2.0 * M_PI * (double)j / (double)N;
            tw[2 * j] = (float)cos(a);
            tw[2 * j + 1] = (float)sin(a);
        }
        ldsp::upload(dtw, tw, dev);
        zero_stream(dev);
        zero_psd(dev);
    }
};

using namespace ldsp;

// Run `fn` translating exceptions into status codes
template <typename F>
static int guard(F&& fn)
{
    try {
        fn();
        return LDSP_OK;
    } catch (const Error& e) {
        set_last_error(e.what());
        return e.code;
    } catch (const std::bad_alloc&) {
        set_last_error("out of host memory");
        return LDSP_ENOMEM;
    } catch (const std::exception& e) {
        set_last_error(e.what());
        return LDSP_EHIP;
    }
}

#define NONNULL(p) LDSP_REQUIRE((p) != nullptr, #p " must not be NULL")

// ---------------------------------------------------------------- per-kernel timing
namespace ldsp {
namespace prof {
namespace {
std::atomic<bool> g_on{false};
std::mutex g_mu;
struct Pending {
    const char* name;
    hipEvent_t a, b;
    hipStream_t s;
};
std::vector<Pending> g_pending;
std::vector<std::pair<std::string, std::pair<long, double>>> g_done;   // name -> (calls, total ms)

// LDSP_PROF_TIMELINE=<file>: also append every profiled launch as
// "name stream start_ms end_ms" relative to the first launch since the last
// reset (overlap and gaps between streams; diagnostics only).
hipEvent_t g_t0 = nullptr;
void drain_locked()
{
    static const char* tl_path = LDSP_KNOB_S("LDSP_PROF_TIMELINE");
    FILE* tl = tl_path ? std::fopen(tl_path, "a") : nullptr;
    for (auto& r : g_pending) {
        float ms = 0.0f;
        if (hipEventSynchronize(r.b) == hipSuccess) (void)hipEventElapsedTime(&ms, r.a, r.b);
        if (tl) {
            if (!g_t0) g_t0 = r.a;
            float t0 = 0.0f;
            (void)hipEventElapsedTime(&t0, g_t0, r.a);
            std::fprintf(tl, "%s %p %.4f %.4f\n", r.name, (void*)r.s, t0, t0 + ms);
        }
        if (r.a != g_t0) (void)hipEventDestroy(r.a);     // the origin lives until the next reset
        (void)hipEventDestroy(r.b);
        auto it = std::find_if(g_done.begin(), g_done.end(), [&](const auto& e) { return e.first == r.name; });
        if (it == g_done.end()) g_done.push_back({r.name, {1, (double)ms}});
        else {
            it->second.first++;
            it->second.second += ms;
        }
    }
    g_pending.clear();
    if (tl) std::fclose(tl);
}
} // namespace

bool enabled() { return g_on.load(std::memory_order_relaxed); }

// ldsp_profile_only: time only the launches of one kernel (the bench's timed
// steps record the dominant kernel alone: two events per launch of it instead
// of two per launch of every kernel)
// The filter points into an interned, never-freed set of names, so a Scope that
// compares against it while another thread changes the filter never reads freed
// memory (the set's nodes do not move).
std::atomic<const char*> g_only{nullptr};
std::set<std::string>* g_only_names = new std::set<std::string>();

Scope::Scope(hipStream_t s_, const char* n) : s(s_), name(n)
{
    // a launcher that issues its kernel directly while a many-call records (batch.hpp)
    // would run it out of order: refuse before the launch
    if (batch_active()) throw Error(LDSP_EUNSUP, std::string("kernel not batchable in a many-call: ") + n);
    if (!enabled()) return;
    const char* only = g_only.load(std::memory_order_relaxed);
    if (only && std::strcmp(only, n) != 0) return;
    if (hipEventCreate(&a) != hipSuccess || hipEventRecord(a, s) != hipSuccess) a = nullptr;
}

Scope::~Scope()
{
    if (!a) return;
    hipEvent_t b = nullptr;
    if (hipEventCreate(&b) != hipSuccess || hipEventRecord(b, s) != hipSuccess) {
        (void)hipEventDestroy(a);
        return;
    }
    std::lock_guard<std::mutex> lk(g_mu);
    g_pending.push_back({name, a, b, s});
    if (g_pending.size() > 4096) drain_locked();
}
} // namespace prof
} // namespace ldsp

extern "C" {

int ldsp_profile_enable(int on)
{
    ldsp::prof::g_on.store(on != 0);
    return LDSP_OK;
}

int ldsp_profile_only(const char* kernel)
{
    return guard([&] {
        std::lock_guard<std::mutex> lk{ldsp::prof::g_mu};
        if (kernel && *kernel)
            ldsp::prof::g_only.store(ldsp::prof::g_only_names->insert(kernel).first->c_str());
        else
            ldsp::prof::g_only.store(nullptr);
    });
}

int ldsp_profile_reset(void)
{
    return guard([&] {
        std::lock_guard<std::mutex> lk{ldsp::prof::g_mu};
        ldsp::prof::drain_locked();
        ldsp::prof::g_done.clear();
        if (ldsp::prof::g_t0) (void)hipEventDestroy(ldsp::prof::g_t0);
        ldsp::prof::g_t0 = nullptr;
    });
}

int ldsp_profile_report(char* buf, size_t cap, size_t* len)
{
    return guard([&] {
        NONNULL(len);
        std::string out;
        {
            std::lock_guard<std::mutex> lk{ldsp::prof::g_mu};
            ldsp::prof::drain_locked();
            char line[256];
            for (const auto& e : ldsp::prof::g_done) {
                std::snprintf(line, sizeof(line), "%s %ld %.6f\n", e.first.c_str(), e.second.first, e.second.second);
                out += line;
            }
        }
        *len = out.size();
        if (buf && cap > 0) {
            const size_t m = std::min(cap - 1, out.size());
            std::memcpy(buf, out.data(), m);
            buf[m] = 0;
        }
    });
}

const char* ldsp_last_error(void) { return g_last_error.c_str(); }
int ldsp_version(void) { return 100; }

int ldsp_device_count(int* n)
{
    return guard([&] {
        NONNULL(n);
        int c = 0;
        if (hipGetDeviceCount(&c) != hipSuccess) c = 0;
        *n = c;
    });
}

int ldsp_stream_synchronize(void* stream)
{
    return guard([&] { LDSP_HIP(hipStreamSynchronize((hipStream_t)stream)); });
}

int ldsp_debug_math_eval(int fn, const float* a, const float* b, float* y, size_t n, void* stream)
{
    return guard([&] {
        LDSP_REQUIRE(fn >= 0 && fn <= 8, "math_eval: unknown function");
        (void)current_device();
        k::math_eval(fn, a, b ? b : a, y, n, (hipStream_t)stream);
    });
}

int ldsp_debug_math_fastcheck(int fn, uint32_t begin, uint32_t end, uint32_t stride, uint64_t* checked,
                              uint64_t* mismatches)
{
    return guard([&] {
        LDSP_REQUIRE(fn >= 0 && fn <= 1 && stride > 0 && checked && mismatches, "math_fastcheck: bad arguments");
        uint64_t c = 0, bad = 0;
        for (uint64_t u = begin; u < end; u += stride) {
            const float a = bitsf((uint32_t)u);
            if (fn == 0) {
                if (lm_logf_fast_ok(a)) {
                    c++;
                    bad += fbits(lm_logf_fast(a)) != fbits(lm_logf(a));
                }
            } else if (fn == 1) {
                if (lm_expf_fast_ok(a)) {
                    c++;
                    bad += fbits(lm_expf_fast(a)) != fbits(lm_expf(a));
                }
            }
        }
        *checked = c;
        *mismatches = bad;
    });
}

// ---------------------------------------------------------------- FIR
static int fir_make(std::vector<float> h, int cplx, ldsp_firfilt_t* q)
{
    LDSP_REQUIRE(!h.empty(), "firfilt: filter length must be > 0");
    LDSP_REQUIRE((int)h.size() <= k::kFirMaxTaps, "firfilt: filter length exceeds 8192 taps");
    auto* o = new ldsp_firfilt_s();
    o->h = std::move(h);
    o->cplx = cplx != 0;
    *q = o;
    return LDSP_OK;
}

int ldsp_firfilt_create(const float* h, unsigned int n, int cplx, ldsp_firfilt_t* q)
{
    return guard([&] {
        NONNULL(q);
        LDSP_REQUIRE(h != nullptr || n == 0, "firfilt: taps must not be NULL");
        fir_make(std::vector<float>(h, h + n), cplx, q);
    });
}

int ldsp_firfilt_create_kaiser(unsigned int n, float fc, float as, float mu, int cplx, ldsp_firfilt_t* q)
{
    return guard([&] {
        NONNULL(q);
        fir_make(design::firdes_kaiser(n, fc, as, mu), cplx, q);
    });
}

int ldsp_firfilt_create_dc_blocker(unsigned int m, float as, int cplx, ldsp_firfilt_t* q)
{
    return guard([&] {
        NONNULL(q);
        fir_make(design::firdes_notch(m, 0.0f, as), cplx, q);
    });
}

int ldsp_firfilt_destroy(ldsp_firfilt_t q) { return guard([&] { destroy(q); }); }

int ldsp_firfilt_reset(ldsp_firfilt_t q)
{
    return guard([&] {
        NONNULL(q);
        if (q->device < 0) return;
        DeviceGuard g(q->device);
        for (auto& b : q->hist.b) LDSP_HIP(hipMemsetAsync(b.p, 0, q->hist_bytes(), q->last));
        q->ord.mark(q->last);              // a call on another stream waits for the zeroing
    });
}

int ldsp_firfilt_set_scale(ldsp_firfilt_t q, float s) { return guard([&] { NONNULL(q); q->scale = s; }); }
int ldsp_firfilt_get_scale(ldsp_firfilt_t q, float* s) { return guard([&] { NONNULL(q); NONNULL(s); *s = q->scale; }); }
int ldsp_firfilt_get_length(ldsp_firfilt_t q, unsigned int* n)
{
    return guard([&] { NONNULL(q); NONNULL(n); *n = (unsigned)q->h.size(); });
}
int ldsp_firfilt_get_taps(ldsp_firfilt_t q, float* h)
{
    return guard([&] { NONNULL(q); NONNULL(h); std::copy(q->h.begin(), q->h.end(), h); });
}
int ldsp_firfilt_set_mode(ldsp_firfilt_t q, int mode)
{
    return guard([&] {
        NONNULL(q);
        LDSP_REQUIRE(mode == LDSP_MODE_FAST || mode == LDSP_MODE_EXACT || mode == LDSP_MODE_DIRECT, "unknown mode");
        q->mode = mode;
    });
}

int ldsp_firfilt_get_mode(ldsp_firfilt_t q, int* mode)
{
    return guard([&] { NONNULL(q); NONNULL(mode); *mode = q->mode; });
}

// liquid firfilt_freqresponse: H = scale * sum_i hrev[i] exp(+j 2 pi f i)
int ldsp_firfilt_freqresponse(ldsp_firfilt_t q, float f, float* re, float* im)
{
    return guard([&] {
        NONNULL(q);
        NONNULL(re);
        NONNULL(im);
        const size_t L = q->h.size();
        std::complex<float> H(0.0f, 0.0f);
        for (size_t i = 0; i < L; i++) {
            const float hr = q->h[L - 1 - i];
            const float ang = (float)(2 * 3.14159265358979323846 * (double)f * (double)i);
            H += hr * std::exp(std::complex<float>(0.0f, ang));
        }
        H *= q->scale;
        *re = H.real();
        *im = H.imag();
    });
}

// One filter call on device buffers, in stream order after the object's
// previous call; `fuse` applies an NCO mix to the samples as the overlap-save
// kernel loads them (only on that path: the caller checks fir_can_fuse).
static void fir_dispatch(ldsp_firfilt_s* q, const void* dx, size_t n, void* dy, hipStream_t s, const k::NcoFuse* fuse)
{
    const int L = (int)q->h.size();
    void* hin = q->hist.in();
    void* hout = q->hist.out();
    if (L <= 1 && n == 0) return;
    const FirObj::Kernel kern = q->kernel_for(n);
    if (kern == FirObj::kExact)
        k::fir_exact(q->cplx, dx, hin, hout, n, q->taps_rev.as<float>(), L, q->scale, dy, s);
    else if (kern == FirObj::kFft) {
        if (!q->fft_ready || q->fft_scale != q->scale) {
            LDSP_HIP(hipStreamSynchronize(s));   // tables may be in use by queued work
            q->prepare_fft();
        }
        k::fir_fft(dx, hin, hout, n, L, q->fft_P(), q->fft_H.p, q->fft_tw.p, dy, s, fuse);
    } else
        k::fir_fast(q->cplx, dx, hin, hout, n, q->taps_pad.as<float>(), L, q->scale, dy, s);
    if (L > 1) q->hist.flip();
}

int ldsp_firfilt_execute(ldsp_firfilt_t q, const void* x, size_t n, void* y, int mem, void* stream)
{
    LDSP_RANGE("ldsp_firfilt_execute");
    return guard([&] {
        NONNULL(q);
        LDSP_REQUIRE(n == 0 || (x && y), "firfilt_execute: NULL buffer");
        Call call(*q, mem, x, stream);
        const Exec& e = call.e;
        const size_t bytes = n * q->esz();
        const void* dx = q->stg.dev_in(e, x, bytes);
        void* dy = q->stg.dev_out(e, y, bytes);
        fir_dispatch(q, dx, n, dy, e.stream, nullptr);
        call.end();
        q->stg.finish(e, y, bytes);
    });
}

// ---------------------------------------------------------------- resampler
// resamp_*_create's filter (ldsp_resamp_create, ldsp_audiobank_create): npfb rounded
// up to a power of two, the Kaiser prototype of 2 m npfb + 1 taps scaled to a DC
// gain of npfb, and its branches reversed, [npfb][sub_len] with c floats per tap
// (c = 2: complex taps, imaginary parts 0)
struct ResampDesign {
    unsigned int npfb = 0, sub_len = 0;
    int bits_index = 0;
    std::vector<float> hproto, sub;
};
static ResampDesign resamp_design(unsigned int m, float fc, float as, unsigned int npfb, unsigned int c)
{
    ResampDesign d;
    unsigned int bits = 0;
    for (unsigned int v = npfb - 1; v; v >>= 1) bits++;   // liquid_nextpow2
    LDSP_REQUIRE(bits <= 16, "resamp: too many filters");
    d.npfb = 1u << bits;
    d.bits_index = 24 - (int)bits;
    const unsigned int n = 2 * m * d.npfb + 1;
    std::vector<float> hf = design::firdes_kaiser(n, fc / ((float)d.npfb), as, 0.0f);
    float gain = 0.0f;
    for (float v : hf) gain += v;
    gain = (float)d.npfb / gain;
    d.hproto.resize(n);
    for (unsigned int i = 0; i < n; i++) d.hproto[i] = hf[i] * gain;
    d.sub_len = (n - 1) / d.npfb;
    d.sub.assign((size_t)d.npfb * d.sub_len * c, 0.0f);
    for (unsigned int b = 0; b < d.npfb; b++)
        for (unsigned int k = 0; k < d.sub_len; k++)
            d.sub[((size_t)b * d.sub_len + (d.sub_len - k - 1)) * c] = d.hproto[b + k * d.npfb];
    return d;
}

int ldsp_resamp_create(float rate, unsigned int m, float fc, float as, unsigned int npfb, int cplx, ldsp_resamp_t* q)
{
    return guard([&] {
        NONNULL(q);
        LDSP_REQUIRE(m > 0, "resamp: filter semi-length must be greater than zero");
        LDSP_REQUIRE(fc > 0.0f && fc < 0.5f, "resamp: filter cutoff must be in (0, 0.5)");
        LDSP_REQUIRE(as > 0.0f, "resamp: filter stop-band suppression must be greater than zero");
        LDSP_REQUIRE(npfb > 0, "resamp: number of filters must be greater than zero");
        LDSP_REQUIRE(cplx >= 0 && cplx <= 2, "resamp: kind must be 0 (rrrf), 1 (cccf) or 2 (crcf)");
        std::unique_ptr<ldsp_resamp_s> o(new ldsp_resamp_s());
        o->cplx = cplx != 0;
        o->real_taps = cplx == 2;
        o->set_rate(rate);
        o->m = m;
        o->fc = fc;
        o->as = as;
        ResampDesign d = resamp_design(m, fc, as, npfb, (o->cplx && !o->real_taps) ? 2 : 1);
        o->npfb = d.npfb;
        o->bits_index = d.bits_index;
        o->sub_len = d.sub_len;
        o->hproto = std::move(d.hproto);
        o->sub = std::move(d.sub);
        *q = o.release();
    });
}

int ldsp_resamp_create_default(float rate, int kind, ldsp_resamp_t* q)
{
    // resamp_*_create_default (liquid resamp.proto.c, recalled): m 7, fc 0.25, As 60, npfb 256
    return ldsp_resamp_create(rate, 7, 0.25f, 60.0f, 256, kind, q);
}

int ldsp_resamp_destroy(ldsp_resamp_t q) { return guard([&] { destroy(q); }); }

int ldsp_resamp_reset(ldsp_resamp_t q)
{
    return guard([&] {
        NONNULL(q);
        q->phase = 0;
        if (q->device < 0) return;
        DeviceGuard g(q->device);
        for (auto& b : q->hist.b) LDSP_HIP(hipMemsetAsync(b.p, 0, q->hist_bytes(), q->last));
        q->ord.mark(q->last);              // a call on another stream waits for the zeroing
    });
}

int ldsp_resamp_set_rate(ldsp_resamp_t q, float rate) { return guard([&] { NONNULL(q); q->set_rate(rate); }); }
int ldsp_resamp_get_rate(ldsp_resamp_t q, float* r) { return guard([&] { NONNULL(q); NONNULL(r); *r = q->rate; }); }
int ldsp_resamp_get_info(ldsp_resamp_t q, unsigned int* npfb, uint32_t* step, uint32_t* phase, unsigned int* sub_len)
{
    return guard([&] {
        NONNULL(q);
        if (npfb) *npfb = q->npfb;
        if (step) *step = q->step;
        if (phase) *phase = (uint32_t)q->phase;
        if (sub_len) *sub_len = q->sub_len;
    });
}
int ldsp_resamp_get_taps(ldsp_resamp_t q, float* h, unsigned int cap, unsigned int* n)
{
    return guard([&] {
        NONNULL(q);
        if (n) *n = (unsigned)q->hproto.size();
        if (h) {
            LDSP_REQUIRE(cap >= q->hproto.size(), "resamp_get_taps: capacity too small");
            std::copy(q->hproto.begin(), q->hproto.end(), h);
        }
    });
}
int ldsp_resamp_num_outputs(ldsp_resamp_t q, size_t n, size_t* nout)
{
    return guard([&] { NONNULL(q); NONNULL(nout); *nout = q->num_outputs(n); });
}

int ldsp_resamp_execute(ldsp_resamp_t q, const void* x, size_t n, void* y, size_t cap, size_t* nout, int mem,
                        void* stream)
{
    LDSP_RANGE("ldsp_resamp_execute");
    return guard([&] {
        NONNULL(q);
        const size_t K = q->num_outputs(n);
        if (nout) *nout = K;
        if (K > cap) throw Error(LDSP_ERANGE, "resamp_execute: output capacity too small");
        LDSP_REQUIRE(n == 0 || x, "resamp_execute: NULL input");
        LDSP_REQUIRE(K == 0 || y, "resamp_execute: NULL output");
        Call call(*q, mem, x, stream);
        const Exec& e = call.e;
        const void* dx = q->stg.dev_in(e, x, n * q->esz());
        void* dy = q->stg.dev_out(e, y, K * q->esz());
        if (n > 0) {
            const k::ResampPlan p = q->plan(n);
            k::resamp(q->cplx, q->real_taps, dx, q->hist.in(), q->hist.out(), n, q->dsub.as<float>(), p, dy, e.stream);
            if (q->sub_len > 1) q->hist.flip();
            q->phase = (uint64_t)((long long)q->phase + (long long)K * q->step - (long long)n * (1LL << 24));
        }
        call.end();
        q->stg.finish(e, y, K * q->esz());
    });
}

// ---------------------------------------------------------------- NCO
int ldsp_nco_create(int type, ldsp_nco_t* q)
{
    return guard([&] {
        NONNULL(q);
        LDSP_REQUIRE(type == 0 || type == 1, "nco: type must be 0 (nco) or 1 (vco)");
        auto* o = new ldsp_nco_s();
        o->type = type;
        o->table = nco_table();
        o->alpha = 0.1f;                     // nco_crcf_pll_set_bandwidth(q, 0.1f) at create
        o->beta = sqrtf(o->alpha);
        *q = o;
    });
}
int ldsp_nco_destroy(ldsp_nco_t q) { return guard([&] { destroy(q); }); }
int ldsp_nco_reset(ldsp_nco_t q) { return guard([&] { NONNULL(q); q->theta = 0; q->dtheta = 0; }); }
int ldsp_nco_set_frequency(ldsp_nco_t q, float f) { return guard([&] { NONNULL(q); q->dtheta = nco_constrain(f); }); }
int ldsp_nco_adjust_frequency(ldsp_nco_t q, float df)
{
    return guard([&] { NONNULL(q); q->dtheta += nco_constrain(df); });
}
int ldsp_nco_set_phase(ldsp_nco_t q, float p) { return guard([&] { NONNULL(q); q->theta = nco_constrain(p); }); }
int ldsp_nco_adjust_phase(ldsp_nco_t q, float dp) { return guard([&] { NONNULL(q); q->theta += nco_constrain(dp); }); }
int ldsp_nco_get_frequency(ldsp_nco_t q, float* f)
{
    return guard([&] {
        NONNULL(q);
        NONNULL(f);
        const double kPi = 3.14159265358979323846;
        const float d = (float)(2.0f * kPi * (double)(float)q->dtheta / (double)(float)(1ULL << 32));
        *f = d > kPi ? (float)(d - 2 * kPi) : d;
    });
}
int ldsp_nco_get_phase(ldsp_nco_t q, float* p)
{
    return guard([&] {
        NONNULL(q);
        NONNULL(p);
        const double kPi = 3.14159265358979323846;
        const float t = (float)(2.0f * kPi * (double)(float)q->theta / (double)(float)(1ULL << 32));
        *p = t > kPi ? (float)(t - 2 * kPi) : t;
    });
}
int ldsp_nco_pll_set_bandwidth(ldsp_nco_t q, float bw)
{
    return guard([&] {
        NONNULL(q);
        LDSP_REQUIRE(bw >= 0.0f, "nco_pll_set_bandwidth: bandwidth must be positive");
        q->alpha = bw;
        q->beta = sqrtf(q->alpha);
    });
}
int ldsp_nco_pll_step(ldsp_nco_t q, float dphi)
{
    return guard([&] {
        NONNULL(q);
        q->dtheta += nco_constrain(dphi * q->alpha);
        q->theta += nco_constrain(dphi * q->beta);
    });
}
int ldsp_nco_get_state(ldsp_nco_t q, uint32_t* t, uint32_t* d)
{
    return guard([&] { NONNULL(q); if (t) *t = q->theta; if (d) *d = q->dtheta; });
}
int ldsp_nco_set_state(ldsp_nco_t q, uint32_t t, uint32_t d)
{
    return guard([&] { NONNULL(q); q->theta = t; q->dtheta = d; });
}

int ldsp_nco_mix(ldsp_nco_t q, const void* x, size_t n, void* y, int down, int mem, void* stream)
{
    LDSP_RANGE("ldsp_nco_mix");
    return guard([&] {
        NONNULL(q);
        LDSP_REQUIRE(n == 0 || (x && y), "nco_mix: NULL buffer");
        Call call(*q, mem, x, stream, false);     // no device state to order: the phase advances on the host
        const Exec& e = call.e;
        const void* dx = q->stg.dev_in(e, x, n * 8);
        void* dy = q->stg.dev_out(e, y, n * 8);
        k::nco_mix(dx, dy, n, q->theta, q->dtheta, q->dtab.as<float>(), down != 0, q->type, e.stream);
        q->theta += (uint32_t)((uint64_t)n * q->dtheta);
        q->stg.finish(e, y, n * 8);
    });
}

// NCO mix fused into the complex FIR (BASELINE config 3): y = fir(nco.mix(x)).
int ldsp_nco_mix_firfilt(ldsp_nco_t nco, ldsp_firfilt_t q, const void* x, size_t n, void* y, int down, int mem,
                         void* stream)
{
    LDSP_RANGE("ldsp_nco_mix_firfilt");
    return guard([&] {
        NONNULL(nco);
        NONNULL(q);
        LDSP_REQUIRE(q->cplx, "nco_mix_firfilt: the filter must be complex (firfilt_crcf / ComplexFIRFilter)");
        LDSP_REQUIRE(n == 0 || (x && y), "nco_mix_firfilt: NULL buffer");
        Call call(*q, *nco, "nco_mix_firfilt: the NCO and the filter live on different devices", mem, x, stream);
        const Exec& e = call.e;
        const size_t bytes = n * 8;
        const void* dx = q->stg.dev_in(e, x, bytes);
        void* dy = q->stg.dev_out(e, y, bytes);
        if (n > 0 && q->use_fft() && nco->type == 0) {
            const k::NcoFuse f{nco->theta, nco->dtheta, down != 0, nco->dtab.as<float>()};
            fir_dispatch(q, dx, n, dy, e.stream, &f);          // the mixed samples never reach HBM
        } else if (n > 0) {
            // other filter modes / the VCO: mix into scratch, then filter (same results)
            void* mb = q->mixbuf.ensure(bytes, q->device);
            k::nco_mix(dx, mb, n, nco->theta, nco->dtheta, nco->dtab.as<float>(), down != 0, nco->type, e.stream);
            fir_dispatch(q, mb, n, dy, e.stream, nullptr);
        } else {
            fir_dispatch(q, dx, 0, dy, e.stream, nullptr);
        }
        nco->theta += (uint32_t)((uint64_t)n * nco->dtheta);
        call.end();
        q->stg.finish(e, y, bytes);
    });
}

// ---------------------------------------------------------------- IIR
static void iir_finalize_sos(ldsp_iirfilt_s* o, const float* B, const float* A, unsigned nsos)
{
    LDSP_REQUIRE(nsos > 0 && nsos <= 8, "iirfilt: 1..8 second-order sections supported");
    o->sos = true;
    o->nsos = nsos;
    o->b.resize(3 * nsos);
    o->a.resize(3 * nsos);
    for (unsigned s = 0; s < nsos; s++) {
        const float a0 = A[3 * s];          // iirfiltsos_set_coefficients
        LDSP_REQUIRE(a0 != 0.0f, "iirfilt: a0 must be non-zero");
        for (int k = 0; k < 3; k++) {
            o->b[3 * s + k] = B[3 * s + k] / a0;
            o->a[3 * s + k] = A[3 * s + k] / a0;
        }
    }
    o->finalize();
}

int ldsp_iirfilt_create_sos(const float* B, const float* A, unsigned int nsos, int cplx, ldsp_iirfilt_t* q)
{
    return guard([&] {
        NONNULL(q);
        NONNULL(B);
        NONNULL(A);
        std::unique_ptr<ldsp_iirfilt_s> o(new ldsp_iirfilt_s());
        o->cplx = cplx != 0;
        iir_finalize_sos(o.get(), B, A, nsos);
        *q = o.release();
    });
}

int ldsp_iirfilt_create_tf(const float* b, unsigned int nb, const float* a, unsigned int na, int cplx,
                           ldsp_iirfilt_t* q)
{
    return guard([&] {
        NONNULL(q);
        LDSP_REQUIRE(b && a && nb > 0 && na > 0, "iirfilt: coefficient arrays must be non-empty");
        LDSP_REQUIRE(nb <= 17 && na <= 17, "iirfilt: transfer functions up to order 16 supported");
        LDSP_REQUIRE(a[0] != 0.0f, "iirfilt: a[0] must be non-zero");
        std::unique_ptr<ldsp_iirfilt_s> o(new ldsp_iirfilt_s());
        o->cplx = cplx != 0;
        o->sos = false;
        o->nb = (int)nb;
        o->na = (int)na;
        o->nv = (int)std::max(nb, na);
        const float a0 = a[0];              // iirfilt_create: normalise by a[0]
        o->b.resize(nb);
        o->a.resize(na);
        for (unsigned i = 0; i < nb; i++) o->b[i] = b[i] / a0;
        for (unsigned i = 0; i < na; i++) o->a[i] = a[i] / a0;
        o->finalize();
        *q = o.release();
    });
}

int ldsp_iirfilt_create_prototype(int ftype, int btype, unsigned int order, float fc, float f0, float ap, float as,
                                  int cplx, ldsp_iirfilt_t* q)
{
    return guard([&] {
        NONNULL(q);
        LDSP_REQUIRE(ftype >= 0 && ftype <= 4, "iirfilt: unknown filter type");
        LDSP_REQUIRE(btype >= 0 && btype <= 3, "iirfilt: unknown band type");
        design::SOS s = design::iirdes_sos(ftype, btype, order, fc, f0, ap, as);
        std::unique_ptr<ldsp_iirfilt_s> o(new ldsp_iirfilt_s());
        o->cplx = cplx != 0;
        iir_finalize_sos(o.get(), s.B.data(), s.A.data(), s.nsos);
        *q = o.release();
    });
}

int ldsp_iirfilt_destroy(ldsp_iirfilt_t q) { return guard([&] { destroy(q); }); }

int ldsp_iirfilt_reset(ldsp_iirfilt_t q)
{
    return guard([&] {
        NONNULL(q);
        if (q->device < 0) return;
        DeviceGuard g(q->device);
        LDSP_HIP(hipMemsetAsync(q->st32.p, 0, q->st32.cap, q->last));
        LDSP_HIP(hipMemsetAsync(q->st64.p, 0, q->st64.cap, q->last));
        if (q->mst.p) LDSP_HIP(hipMemsetAsync(q->mst.p, 0, q->mst.cap, q->last));
        q->ord.mark(q->last);              // a call on another stream waits for the zeroing
    });
}

int ldsp_iirfilt_set_mode(ldsp_iirfilt_t q, int mode)
{
    return guard([&] {
        NONNULL(q);
        LDSP_REQUIRE(mode == LDSP_MODE_FAST || mode == LDSP_MODE_EXACT, "unknown mode");
        q->mode = mode;
    });
}
int ldsp_iirfilt_get_nsos(ldsp_iirfilt_t q, unsigned int* n)
{
    return guard([&] { NONNULL(q); NONNULL(n); *n = q->sos ? q->nsos : 0; });
}
int ldsp_debug_iir_path(ldsp_iirfilt_t q, int path)
{
    return guard([&] {
        NONNULL(q);
        LDSP_REQUIRE(path >= 0 && path <= 3,
                     "iirfilt: path must be 0 (automatic), 1 (blocked scan), 2 (modal) or 3 (modal, look-back recomputed)");
        LDSP_REQUIRE(path < 2 || q->mf.ok, "iirfilt: this filter has no valid modal form");
        q->path_force = path;
    });
}
int ldsp_debug_agc_tsa_perturb(ldsp_agc_t q, int on)
{
    return guard([&] {
        NONNULL(q);
        q->tsa_perturb = on ? 1 : 0;
    });
}
int ldsp_debug_agc_perturb(ldsp_agc_t q, int on)
{
    return guard([&] {
        NONNULL(q);
        q->perturb = on ? 1 : 0;
    });
}
int ldsp_debug_agc_rounds(ldsp_agc_t q, int rounds)
{
    return guard([&] {
        NONNULL(q);
        LDSP_REQUIRE(rounds >= -1 && rounds <= 6, "agc: rounds must be -1 (default) or 0..6");
        q->rounds_force = rounds;
    });
}
int ldsp_debug_agc_reruns(ldsp_agc_t q, unsigned int* runfix, unsigned int* verify)
{
    return guard([&] {
        NONNULL(q);
        q->pull();
        if (runfix) *runfix = (unsigned)q->h.pad[2];
        if (verify) *verify = (unsigned)q->h.pad[1];
    });
}
int ldsp_debug_agc_tsa_reruns(ldsp_agc_t q, unsigned int* count)
{
    return guard([&] {
        NONNULL(q);
        NONNULL(count);
        q->pull();
        *count = (unsigned)q->h.pad[0];
    });
}
int ldsp_debug_iir_modal_info(ldsp_iirfilt_t q, int* ok, int* modes, int* lookback, double* err)
{
    return guard([&] {
        NONNULL(q);
        if (ok) *ok = q->mf.ok ? 1 : 0;
        if (modes) *modes = q->mf.M;
        if (lookback) *lookback = q->mf.J;
        if (err) *err = q->mf.err;
    });
}
int ldsp_debug_iir_modal_grid(ldsp_iirfilt_t q, size_t n, long* units, int* one_xcd, unsigned int* grid)
{
    return guard([&] {
        NONNULL(q);
        LDSP_REQUIRE(q->mf.ok, "iirfilt: this filter has no valid modal form");
        const int onex = q->modal_one_xcd(n);
        if (units) *units = k::iir_modal_units(n);
        if (one_xcd) *one_xcd = onex;
        if (grid) *grid = k::iir_modal_grid(n, onex);
    });
}
int ldsp_debug_iir_dispatch(ldsp_iirfilt_t q, size_t n, int* path, int* sect_tile, int* size_class, int* spec_W,
                            int* spec_staged)
{
    return guard([&] {
        NONNULL(q);
        const IirObj::Path p = q->path_for(n);
        const k::IirSeqKernel kq = k::iir_seq_kernel(q->desc());
        if (path) *path = (int)p;
        if (sect_tile) *sect_tile = p == IirObj::kSeq ? kq.sect_tile : 0;
        if (size_class) *size_class = kq.size_class;
        if (spec_W) *spec_W = q->spec_W;
        if (spec_staged) *spec_staged = p == IirObj::kSpec && k::iir_spec_staged(q->cplx, q->spec_plan(n)) ? 1 : 0;
    });
}
int ldsp_debug_fir_dispatch(ldsp_firfilt_t q, size_t n, int* kernel, int* points, int* overlap)
{
    return guard([&] {
        NONNULL(q);
        const FirObj::Kernel kern = q->kernel_for(n);
        if (kernel) *kernel = (int)kern;
        if (points) *points = kern == FirObj::kFft ? k::fir_fft_points(q->fft_P()) : 0;
        if (overlap) *overlap = kern == FirObj::kFft ? q->fft_P() : 0;
    });
}
int ldsp_debug_resamp_dispatch(ldsp_resamp_t q, size_t n, int* kernel, int* outputs_per_group)
{
    return guard([&] {
        NONNULL(q);
        const k::ResampPlan p = q->plan(n);
        const k::ResampKernel kern = k::resamp_kernel(p, q->cplx, q->real_taps);
        if (kernel) *kernel = (int)kern;
        if (outputs_per_group) *outputs_per_group = kern == k::kResampDirect ? k::kResampDirectOutputs : p.KB;
    });
}
int ldsp_iirfilt_get_sos(ldsp_iirfilt_t q, float* B, float* A)
{
    return guard([&] {
        NONNULL(q);
        LDSP_REQUIRE(q->sos, "iirfilt_get_sos: filter is in transfer-function form");
        if (B) std::copy(q->b.begin(), q->b.end(), B);
        if (A) std::copy(q->a.begin(), q->a.end(), A);
    });
}

// liquid iirfilt_freqresponse (evaluates with exp(+j 2 pi f k))
int ldsp_iirfilt_freqresponse(ldsp_iirfilt_t q, float f, float* re, float* im)
{
    return guard([&] {
        NONNULL(q);
        NONNULL(re);
        NONNULL(im);
        using cf = std::complex<float>;
        const double kPi = 3.14159265358979323846;
        auto ex = [&](int k) { return std::exp(cf(0.0f, (float)(2 * kPi * (double)f * (double)k))); };
        cf H;
        if (!q->sos) {
            cf Ha(0.0f, 0.0f), Hb(0.0f, 0.0f);
            for (int i = 0; i < q->nb; i++) Hb += q->b[i] * ex(i);
            for (int i = 0; i < q->na; i++) Ha += q->a[i] * ex(i);
            H = Hb / Ha;
        } else {
            H = cf(1.0f, 0.0f);
            for (unsigned s = 0; s < q->nsos; s++) {
                const cf Hb = q->b[3 * s] * ex(0) + q->b[3 * s + 1] * ex(1) + q->b[3 * s + 2] * ex(2);
                const cf Ha = q->a[3 * s] * ex(0) + q->a[3 * s + 1] * ex(1) + q->a[3 * s + 2] * ex(2);
                H *= Hb / Ha;
            }
        }
        *re = H.real();
        *im = H.imag();
    });
}

// iq16: x is n int16 (I, Q) pairs (bytes_to_iq's input); the blocked float64
// scan converts them on load, the other paths after a k_bytes_to_iq pass.
static int iirfilt_execute(ldsp_iirfilt_t q, const void* x, size_t n, void* y, int mem, void* stream, bool iq16)
{
    return guard([&] {
        NONNULL(q);
        LDSP_REQUIRE(n == 0 || (x && y), "iirfilt_execute: NULL buffer");
        LDSP_REQUIRE(!iq16 || q->cplx, "iirfilt_execute_iq16: the filter is real; int16 IQ input needs a complex one");
        Call call(*q, mem, x, stream);
        const Exec& e = call.e;
        const size_t bytes = n * (q->cplx ? 8 : 4);
        const void* dx = q->stg.dev_in(e, x, iq16 ? n * 4 : bytes);
        void* dy = q->stg.dev_out(e, y, bytes);
        if (n > 0) {
            const k::IirDesc d = q->desc();
            using P = IirObj::Path;
            const P path = q->path_for(n);
            enum { kSpec = P::kSpec, kSeq = P::kSeq, kModal = P::kModal, kBlk = P::kBlk, kScan = P::kScan };
            if (iq16 && path != kModal && path != kBlk) {   // not fused: convert first
                void* cx = q->iq.ensure(n * 8, q->device);
                k::bytes_to_iq(dx, cx, n, e.stream);
                dx = cx;
                iq16 = false;
            }
            switch (path) {
            case kSpec: {   // speculative exact chunks (same bits as sequential)
                q->state_to(IirObj::kSt32, e.stream);
                k::SpecPlan p = q->spec_plan(n);
                const size_t need = k::spec_scratch_bytes(p.nchunks, q->ncomp(), q->fsz());
                p.scratch = q->sc1.ensure(need, q->device);
                k::iir_spec(q->cplx, d, dx, n, q->st32.as<float>(), p, dy, e.stream);
                break;
            }
            case kSeq:
                q->state_to(IirObj::kSt32, e.stream);
                k::iir_seq(q->cplx, d, dx, n, q->st32.as<float>(), dy, e.stream);
                break;
            case kModal: {  // one pass: reads mst (the call's start), writes mstb (its end); then swap
                q->state_to(IirObj::kStModal, e.stream);
                const k::IirModalPlan p = q->modal_plan(n);
                k::iir_modal(q->cplx, q->mf.cf, dx, n, q->mst.as<double>(), q->mstb.as<double>(), p, dy, e.stream,
                             iq16);
                std::swap(q->mst.p, q->mstb.p);
                std::swap(q->mst.cap, q->mstb.cap);
                break;
            }
            case kBlk: {
                q->state_to(IirObj::kSt64, e.stream);
                const k::IirBlkPlan p = q->blk_plan(n);
                k::iir_blk(q->cplx, d, q->b.data(), q->a.data(), dx, n, q->st64.as<double>(), p, dy, e.stream, iq16);
                break;
            }
            case kScan: {
                q->state_to(IirObj::kSt64, e.stream);
                const k::IirScanPlan p = q->scan_plan(n);
                k::iir_scan(q->cplx, d, dx, n, q->st64.as<double>(), p, dy, e.stream);
                break;
            }
            }
        }
        call.end();
        q->stg.finish(e, y, bytes);
    });
}
int ldsp_iirfilt_execute(ldsp_iirfilt_t q, const void* x, size_t n, void* y, int mem, void* stream)
{
    LDSP_RANGE("ldsp_iirfilt_execute");
    return iirfilt_execute(q, x, n, y, mem, stream, false);
}
int ldsp_iirfilt_execute_iq16(ldsp_iirfilt_t q, const void* x, size_t n, void* y, int mem, void* stream)
{
    LDSP_RANGE("ldsp_iirfilt_execute_iq16");
    return iirfilt_execute(q, x, n, y, mem, stream, true);
}

// IIR -> resampler (resamp(iirfilt(x))) in one pass when the filter takes the
// modal scan: the filter outputs stay on chip (k_iir_modal<RS>), the resampler
// outputs are the resampler kernels' bits, and both objects' states advance as
// after the two calls.  Any other configuration runs the two calls.
int ldsp_iirfilt_resamp_execute(ldsp_iirfilt_t q, ldsp_resamp_t rs, const void* x, size_t n, void* y, size_t cap,
                                size_t* nout, int mem, void* stream)
{
    LDSP_RANGE("ldsp_iirfilt_resamp_execute");
    return guard([&] {
        NONNULL(q);
        NONNULL(rs);
        LDSP_REQUIRE(q->cplx == rs->cplx, "iirfilt_resamp_execute: the filter and the resampler must both be complex "
                                          "or both real");
        const size_t K = rs->num_outputs(n);
        if (nout) *nout = K;
        if (K > cap) throw Error(LDSP_ERANGE, "iirfilt_resamp_execute: output capacity too small");
        LDSP_REQUIRE(n == 0 || x, "iirfilt_resamp_execute: NULL input");
        LDSP_REQUIRE(K == 0 || y, "iirfilt_resamp_execute: NULL output");
        // (each path below orders both objects itself: the two calls do, the fused pass waits for and marks both)
        Call call(*q, *rs, "iirfilt_resamp_execute: the filter and the resampler live on different devices", mem, x,
               stream, false);
        const Exec& e = call.e;
        const size_t es = q->cplx ? 8 : 4;
        const bool fuse = n > 0 && q->path_for(n) == IirObj::kModal && rs->sub_len >= 2 &&
                          rs->sub_len - 1 <= 1024u;
        if (!fuse) {
            if (e.host) {
                // the hand-over in page-locked memory when the pool has it (the two
                // calls then DMA it directly), pageable otherwise; the caller's stream
                const size_t tb = std::max<size_t>(n, 1) * es;
                void* tp = nullptr;
                std::vector<char> tv;
                if (ldsp_host_alloc(tb, &tp) != LDSP_OK) {
                    tp = nullptr;
                    tv.resize(tb);
                }
                struct Free {
                    void* p;
                    ~Free() { if (p) (void)ldsp_host_free(p); }
                } fr{tp};
                void* t = tp ? tp : tv.data();
                ok(ldsp_iirfilt_execute(q, x, n, t, LDSP_MEM_HOST, stream));
                ok(ldsp_resamp_execute(rs, t, n, y, cap, nout, LDSP_MEM_HOST, stream));
            } else {
                void* t = q->rsbuf.ensure(std::max<size_t>(n, 1) * es, q->device);
                ok(ldsp_iirfilt_execute(q, x, n, t, LDSP_MEM_DEVICE, stream));
                ok(ldsp_resamp_execute(rs, t, n, y, cap, nout, LDSP_MEM_DEVICE, stream));
                q->ord.mark(e.stream);            // the next filter call rewrites t only after the resampler read it
            }
            return;
        }
        q->ord.wait(e.stream);
        rs->ord.wait(e.stream);
        const void* dx = q->stg.dev_in(e, x, n * es);
        void* dy = rs->stg.dev_out(e, y, K * es);
        q->state_to(IirObj::kStModal, e.stream);
        const k::IirModalPlan p = q->modal_plan(n);
        k::IirResampFuse f;
        f.sub = rs->dsub.as<float>();
        f.P0 = rs->phase;
        f.step = rs->step;
        f.bits_index = rs->bits_index;
        f.sub_len = (int)rs->sub_len;
        f.ctaps = (rs->cplx && !rs->real_taps) ? 1 : 0;
        f.K = (long)K;
        f.side = (float*)q->rsside.ensure(k::iir_resamp_side_bytes(n, (int)rs->sub_len, q->cplx), q->device);
        f.y = (float*)dy;
        k::iir_modal_resamp(q->cplx, q->mf.cf, dx, n, q->mst.as<double>(), q->mstb.as<double>(), p, f,
                            rs->hist.in(), rs->hist.out(), e.stream);
        std::swap(q->mst.p, q->mstb.p);
        std::swap(q->mst.cap, q->mstb.cap);
        rs->hist.flip();
        rs->phase = (uint64_t)((long long)rs->phase + (long long)K * rs->step - (long long)n * (1LL << 24));
        q->ord.mark(e.stream);
        rs->ord.mark(e.stream);
        call.end();
        rs->last = e.stream;
        rs->stg.finish(e, y, K * es);
    });
}

// ---------------------------------------------------------------- AGC
int ldsp_agc_create(ldsp_agc_t* q)
{
    return guard([&] {
        NONNULL(q);
        auto* o = new ldsp_agc_s();
        o->init();
        *q = o;
    });
}
int ldsp_agc_destroy(ldsp_agc_t q) { return guard([&] { destroy(q); }); }

// agc_crcf_reset: g = 1, y2' = 1, unlock, squelch ENABLED unless disabled
int ldsp_agc_reset(ldsp_agc_t q)
{
    return guard([&] {
        NONNULL(q);
        q->pull();
        q->h.g = 1.0f;
        q->h.y2p = 1.0f;
        q->h.locked = 0;
        q->h.mode = (q->h.mode == 7) ? 7 : 1;
        q->modified();
    });
}
int ldsp_agc_set_bandwidth(ldsp_agc_t q, float bw)
{
    return guard([&] {
        NONNULL(q);
        LDSP_REQUIRE(bw >= 0.0f && bw <= 1.0f, "agc_set_bandwidth: bandwidth must be in [0, 1]");
        q->pull();
        q->bandwidth = bw;
        q->h.alpha = bw;
        q->modified();
    });
}
int ldsp_agc_get_bandwidth(ldsp_agc_t q, float* bw) { return guard([&] { NONNULL(q); NONNULL(bw); *bw = q->bandwidth; }); }
int ldsp_agc_lock(ldsp_agc_t q, int on)
{
    return guard([&] { NONNULL(q); q->pull(); q->h.locked = on ? 1 : 0; q->modified(); });
}
int ldsp_agc_squelch_enable(ldsp_agc_t q, int on)
{
    return guard([&] { NONNULL(q); q->pull(); q->h.mode = on ? 1 : 7; q->modified(); });
}
int ldsp_agc_squelch_set_threshold(ldsp_agc_t q, float t)
{
    return guard([&] { NONNULL(q); q->pull(); q->h.threshold = t; q->modified(); });
}
int ldsp_agc_squelch_get_threshold(ldsp_agc_t q, float* t)
{
    return guard([&] { NONNULL(q); NONNULL(t); *t = q->h.threshold; });
}
int ldsp_agc_squelch_set_timeout(ldsp_agc_t q, unsigned int t)
{
    return guard([&] { NONNULL(q); q->pull(); q->h.timeout = t; q->modified(); });
}
int ldsp_agc_squelch_get_status(ldsp_agc_t q, int* s)
{
    return guard([&] { NONNULL(q); NONNULL(s); q->pull(); *s = q->h.mode; });
}
int ldsp_agc_get_gain(ldsp_agc_t q, float* g) { return guard([&] { NONNULL(q); NONNULL(g); q->pull(); *g = q->h.g; }); }
int ldsp_agc_set_gain(ldsp_agc_t q, float g)
{
    return guard([&] {
        NONNULL(q);
        LDSP_REQUIRE(g > 0.0f, "agc_set_gain: gain must be greater than zero");
        q->pull();
        q->h.g = g;
        q->modified();
    });
}
int ldsp_agc_get_scale(ldsp_agc_t q, float* s) { return guard([&] { NONNULL(q); NONNULL(s); *s = q->h.scale; }); }
int ldsp_agc_set_scale(ldsp_agc_t q, float s)
{
    return guard([&] {
        NONNULL(q);
        LDSP_REQUIRE(s > 0.0f, "agc_set_scale: scale must be greater than zero");
        q->pull();
        q->h.scale = s;
        q->modified();
    });
}
int ldsp_agc_get_signal_level(ldsp_agc_t q, float* x)
{
    return guard([&] { NONNULL(q); NONNULL(x); q->pull(); *x = (float)(1.0 / (double)q->h.g); });
}
int ldsp_agc_set_signal_level(ldsp_agc_t q, float x)
{
    return guard([&] {
        NONNULL(q);
        LDSP_REQUIRE(x > 0.0f, "agc_set_signal_level: level must be greater than zero");
        q->pull();
        q->h.g = (float)(1.0 / (double)x);
        q->h.y2p = 1.0f;
        q->modified();
    });
}
int ldsp_agc_get_rssi(ldsp_agc_t q, float* r)
{
    return guard([&] { NONNULL(q); NONNULL(r); q->pull(); *r = (float)(-20 * log10((double)q->h.g)); });
}
int ldsp_agc_set_rssi(ldsp_agc_t q, float r)
{
    return guard([&] {
        NONNULL(q);
        q->pull();
        q->h.g = powf(10.0f, -r / 20.0f);
        if (q->h.g < 1e-16f) q->h.g = 1e-16f;
        q->h.y2p = 1.0f;
        q->modified();
    });
}
int ldsp_agc_set_mode(ldsp_agc_t q, int mode)
{
    return guard([&] {
        NONNULL(q);
        LDSP_REQUIRE(mode == LDSP_MODE_FAST || mode == LDSP_MODE_EXACT, "unknown mode");
    });
}

// The path of a call of n samples (ldsp_agc_execute, ldsp_debug_agc_dispatch):
// host logic only, nothing of the object changes.
struct AgcChoice {
    enum Path { kSeq = 0, kTsa = 1, kPar = 2 };
    int path = kSeq;                  // sequential loop, small-call chunks from the true state, chunk-parallel
    int W = 0, Wa = 0;                // exact and approximate warm-up lengths of this bandwidth
    int C = 0;                        // chunk length (0: sequential)
    long nchunks = 0;
    long hist_len = 0;                // input history a speculative call needs: W + Wa + kAgcPow
    bool spec = false;                // chunk-parallel from the history alone (front, repair, verify)
};
static AgcChoice agc_choice(const AgcObj* q, size_t n)
{
    AgcChoice ch;
    // exact warm-up W = 5/bandwidth after an approximate one of Wa = 40/bandwidth
    // (k_agc.hip); measured on the AM chain at bandwidth 0.01 the exact loop then
    // coalesces within ~110 samples on average, 2834 at worst.  The chunks that
    // have not by then (~70 of 1 573 per 64 Mi call at W = 5/bw, 7 at 20/bw) go
    // to the windowed one-wave run-fix, which stops at the first checkpoint that
    // meets the stored trajectory: single call 3.72 -> 3.42 ms against W = 20/bw
    // (W = 3/bw: 3.71, more runs), 20-step and batched channels unchanged.
    const float a = q->h.alpha > 1e-6f ? q->h.alpha : 1e-6f;
    static const float wmul = LDSP_KNOB_F("LDSP_AGC_WMUL", 5.0f);
    static const float wamul = LDSP_KNOB_F("LDSP_AGC_WAMUL", 40.0f);
    static const bool nospec = LDSP_KNOB("LDSP_AGC_NOSPEC", 0) != 0;   // A/B: every call from the true state
    const int W = (int)std::min(1 << 18, std::max(256, (int)(wmul / a)));
    const int Wa = (int)std::min(1 << 20, std::max(1024, (int)(wamul / a)));
    ch.W = W;
    ch.Wa = Wa;
    ch.hist_len = (long)W + Wa + k::kAgcPow;
    // Latency per step on one lane (scripts/ubench/loop_lat.hip): approximate
    // 0.06 us, exact 0.25 us.  Chunk-parallel from guesses (every chunk Wa
    // approximate + W + 256 exact steps, ~0.8 us at bandwidth 0.01, overlapping
    // the previous call) once a call is long enough that the true-start chunks
    // below would take more than half of that.
    static const size_t parmin = (size_t)LDSP_KNOB("LDSP_AGC_PARMIN", 0L);
    const bool par = n >= (parmin ? parmin : std::max<size_t>(2048, (size_t)(0.5 * (0.06 * Wa + 0.25 * (W + 256)) / 0.06)));
    // below that, from ~300 samples: chunks approximating from the true state
    // (latency 0.06 us per sample before the last chunk + 256 exact steps)
    static const size_t tsamin = (size_t)LDSP_KNOB("LDSP_AGC_TSAMIN", 320L);
    const bool tsa = !par && n >= tsamin;
    ch.path = par ? AgcChoice::kPar : tsa ? AgcChoice::kTsa : AgcChoice::kSeq;
    // a changed bandwidth (another hist_len) restarts the history
    const long valid = ch.hist_len == q->hist_len ? q->hist_valid : 0;
    ch.spec = !nospec && !tsa && valid >= ch.hist_len;
    if (n > 0 && (par || tsa)) {
        // chunk length: every chunk re-runs Wa + W warm-up steps (6 000 at
        // bandwidth 0.01) for its C outputs, so C = 1024 does a quarter of the
        // front's work of C = 256 at ~20 % more latency (hidden under the PLL
        // walk in a streamed chain); measured on 8 channels per GPU 6.6 -> 6.3
        // ms per step (scripts/agc_chunk_sweep.sh).  Small calls (tsa): the
        // one wave runs the approximate loop up to the last chunk's start and
        // then C exact steps, so the shortest chunks that still fit 64 lanes
        // (C >= 32) cut the exact tail: a README call (1 573 samples) 256 -> 32
        // exact steps after the same approximate run.  Multi-wave tsa calls keep 256.
        static const int agc_c = LDSP_KNOB("LDSP_AGC_C", 1024);
        static const int tsa_cmin = LDSP_KNOB("LDSP_AGC_TSA_CMIN", 32);
        const int c64 = (int)(((n + 63) / 64 + 31) / 32 * 32);      // 64 chunks of a multiple of 32
        ch.C = tsa ? (c64 <= 256 ? std::max(tsa_cmin, c64) : 256) : agc_c;
        ch.nchunks = (long)((n + ch.C - 1) / ch.C);
    }
    return ch;
}

// Two halves per call (k_agc.hip): the front runs the speculative chunks --
// from the input history alone once it holds hist_len samples, so call k + 1's
// front overlaps call k's back half on another stream -- and the back half
// checks chunk 0 against the true state, repairs and verifies, and advances it.
int ldsp_agc_execute(ldsp_agc_t q, const void* x, size_t n, void* y, uint8_t* status, int mem, void* stream)
{
    LDSP_RANGE("ldsp_agc_execute");
    return guard([&] {
        NONNULL(q);
        LDSP_REQUIRE(n == 0 || (x && y), "agc_execute: NULL buffer");
        Call call(*q, mem, x, stream, false);     // the halves order themselves: front / slot[] here, ord between them
        const Exec& e = call.e;
        const int sl = (int)(q->ncall & 1), h3 = (int)(q->ncall % 3);
        q->slot[sl].wait(e.stream);
        q->front.wait(e.stream);
        if (q->upload_pending) {
            q->ord.wait(e.stream);
            LDSP_HIP(hipStreamSynchronize(e.stream));
            LDSP_HIP(hipMemcpy(q->dst.p, &q->h, sizeof(q->h), hipMemcpyHostToDevice));
            q->upload_pending = false;
        }
        const void* dx = q->stg.dev_in(e, x, n * 8);
        void* dy = q->stg.dev_out(e, y, n * 8);
        uint8_t* dstat = status ? (uint8_t*)q->status.ensure(std::max<size_t>(n, 1), q->device) : nullptr;
        // exact warm-up W = 5/bandwidth after an approximate one of Wa = 40/bandwidth
        // (k_agc.hip); measured on the AM chain at bandwidth 0.01 the exact loop then
        // coalesces within ~110 samples on average, 2834 at worst.  The chunks that
        // have not by then (~70 of 1 573 per 64 Mi call at W = 5/bw, 7 at 20/bw) go
        // to the windowed one-wave run-fix, which stops at the first checkpoint that
        // meets the stored trajectory: single call 3.72 -> 3.42 ms against W = 20/bw
        // (W = 3/bw: 3.71, more runs), 20-step and batched channels unchanged
        // (gpurun_out r05zo).
        // repair rounds (flag + run-by-run re-run launches) before the one-wave
        // verifier, which re-runs whatever a round left: on the bench chain every
        // repair lands in round 1 (rounds 2-3 found nothing), and with 8 channels
        // per GPU each launch on a chain waits 0.1-0.2 ms for a slot, so one round
        // (8 channels 5.62-5.78 vs 5.83-6.24 ms per step, profiles/r04v_channels.txt)
        static const int rounds = LDSP_KNOB("LDSP_AGC_ROUNDS", 1);
        const AgcChoice ch = agc_choice(q, n);
        const int W = ch.W, Wa = ch.Wa;
        const long hl = ch.hist_len;
        if (hl != q->hist_len) {             // bandwidth changed: history restarts
            q->hist_len = hl;
            q->hist_valid = 0;
            for (int i = 0; i < 3; i++) q->hist[i].ensure((size_t)hl * 8, q->device);
        }
        const bool par = ch.path == AgcChoice::kPar, tsa = ch.path == AgcChoice::kTsa, spec = ch.spec;
        k::SpecPlan p;
        if (n > 0 && (par || tsa)) {
            p.W = tsa ? 0 : W;                 // tsa: every chunk from 1 on is checked against its predecessor
            p.Wa = Wa;
            p.rounds = tsa ? 1 : std::max(0, std::min(q->rounds_force >= 0 ? q->rounds_force : rounds, 6));
            // (tsa: one run covers the rare deviation)
            p.C = ch.C;
            p.nchunks = ch.nchunks;
            p.scratch = q->scr[sl].ensure(k::agc_scratch_bytes(p.nchunks, p.C), q->device);
            p.hist = q->hist[h3].p;
            p.H = spec ? (int)hl : 0;
            // a small call's chunks in one wave check and repair themselves (tsa 2:
            // no flag / repair / verify launches on the call's critical path)
            static const bool tsa_sep = LDSP_KNOB("LDSP_AGC_TSA_SEPARATE", 0) != 0;
            p.tsa = tsa ? (p.nchunks <= 64 && !tsa_sep && !LDSP_KNOB("LDSP_DEBUG_AGC", 0) ? 2 : 1) : 0;
            if (p.tsa == 2 && q->tsa_perturb) p.tsa |= 4;
            if (!tsa && q->perturb) p.tsa |= 8;          // test hook: odd chunks start 1 ulp off
        }
        // the next call's history first: its front then waits for this copy only
        if (n > 0) k::delay_hist(dx, q->hist[h3].p, q->hist[(h3 + 1) % 3].p, n, (int)hl, e.stream);
        q->front.mark(e.stream);
        static const bool dbg = LDSP_KNOB("LDSP_DEBUG_AGC", 0) != 0;    // per-round re-run counters
        if (n > 0 && (par || tsa)) {
            if (dbg) {
                p.dbg = (unsigned*)p.scratch + (size_t)p.nchunks * 8;
                LDSP_HIP(hipMemsetAsync(p.dbg, 0, 8 * sizeof(unsigned), e.stream));
            }
            if (!spec) q->ord.wait(e.stream);         // chunks near the start read the true state
            k::agc_spec_front(dx, n, q->dst.as<k::AgcState>(), p, dy, dstat, e.stream);
            // speculative call: the repair rounds need no true state (off the chain between calls)
            if (spec) k::agc_spec_repair(dx, n, q->dst.as<k::AgcState>(), p, dy, dstat, e.stream);
        }
        q->ord.wait(e.stream);
        if (n > 0) {
            if (par || tsa) {
                if (spec) k::agc_spec_verify(dx, n, q->dst.as<k::AgcState>(), p, dy, dstat, e.stream);
                else if (!(p.tsa & 2)) k::agc_spec_back(dx, n, q->dst.as<k::AgcState>(), p, dy, dstat, e.stream);
                if (dbg) {
                    unsigned c[8];
                    LDSP_HIP(hipMemcpyAsync(c, p.dbg, sizeof(c), hipMemcpyDeviceToHost, e.stream));
                    LDSP_HIP(hipStreamSynchronize(e.stream));
                    std::fprintf(stderr, "[ldsp agc] n=%zu chunks=%ld W=%d Wa=%d spec=%d rounds=%d reruns per round:", n,
                                 p.nchunks, p.W, p.Wa, spec ? 1 : 0, p.rounds);
                    for (int r = 0; r <= p.rounds; r++) std::fprintf(stderr, " %u", c[r]);
                    std::fprintf(stderr, " (last = verifier)\n");
                }
            } else {
                k::agc_seq(dx, n, q->dst.as<k::AgcState>(), dy, dstat, e.stream);
            }
            q->dev_newer = true;
            q->hist_valid = std::min<long>(hl, q->hist_valid + (long)n);
        }
        q->ord.mark(e.stream);
        q->slot[sl].mark(e.stream);
        q->ncall++;
        call.end();
        if (status && n > 0) {
            LDSP_HIP(hipMemcpyAsync(status, dstat, n, hipMemcpyDeviceToHost, e.stream));
            LDSP_HIP(hipStreamSynchronize(e.stream));
        }
        q->stg.finish(e, y, n * 8);
    });
}

int ldsp_debug_agc_dispatch(ldsp_agc_t q, size_t n, int* path, int* W, int* Wa, int* C, long* hist_len,
                            long* hist_valid, int* spec)
{
    return guard([&] {
        NONNULL(q);
        const AgcChoice ch = agc_choice(q, n);
        if (path) *path = ch.path;
        if (W) *W = ch.W;
        if (Wa) *Wa = ch.Wa;
        if (C) *C = ch.C;
        if (hist_len) *hist_len = ch.hist_len;
        if (hist_valid) *hist_valid = ch.hist_len == q->hist_len ? q->hist_valid : 0;
        if (spec) *spec = ch.spec ? 1 : 0;
    });
}

// ---------------------------------------------------------------- AmpModem
int ldsp_ampmodem_create(float mod_index, int type, int suppressed_carrier, ldsp_ampmodem_t* q)
{
    return guard([&] {
        NONNULL(q);
        LDSP_REQUIRE(type >= 0 && type <= 2, "ampmodem: type must be 0 (dsb), 1 (usb) or 2 (lsb)");
        std::unique_ptr<ldsp_ampmodem_s> o(new ldsp_ampmodem_s());
        o->mod_index = mod_index;
        o->type = type;
        o->suppressed = suppressed_carrier != 0;
        o->m = 25;
        o->lp = design::firdes_kaiser(2 * o->m + 1, 0.01f, 40.0f, 0.0f);   // carrier lowpass
        o->dc = design::firdes_notch(o->m, 0.0f, 20.0f);                     // DC blocker
        if (type != 0) o->hq = design::firhilb_taps(o->m, 60.0f);            // firhilbf_create(m, 60)
        o->table = nco_table();
        o->reset_host();
        *q = o.release();
    });
}
int ldsp_ampmodem_destroy(ldsp_ampmodem_t q) { return guard([&] { destroy(q); }); }
static void amp_reset(AmpObj* q)
{
    q->reset_host();
    q->dev_newer = false;
    if (q->device < 0) return;
    DeviceGuard g(q->device);
    q->sync_all();
    q->st.wepoch = q->wexp;               // every issued launch has published: the epoch stands
    q->st.werr = 0;
    if (q->herr) __atomic_store_n(q->herr, 0u, __ATOMIC_RELEASE);
    LDSP_HIP(hipMemcpy(q->dst.p, &q->st, sizeof(q->st), hipMemcpyHostToDevice));
    for (PingPong* h : {&q->lph, &q->dch, &q->hbh})
        for (auto& b : h->b)
            if (b.p) zero_now(b.p, 0, b.cap);
    for (auto& b : q->dlh)
        if (b.p) zero_now(b.p, 0, b.cap);
    q->hbh.cur = 0;
}
int ldsp_ampmodem_reset(ldsp_ampmodem_t q)
{
    return guard([&] {
        NONNULL(q);
        amp_reset(q);
    });
}
int ldsp_ampmodem_get_taps(ldsp_ampmodem_t q, float* lowpass, float* dcblock, float* hilbert)
{
    return guard([&] {
        NONNULL(q);
        if (lowpass) std::copy(q->lp.begin(), q->lp.end(), lowpass);
        if (dcblock) std::copy(q->dc.begin(), q->dc.end(), dcblock);
        if (hilbert) {
            const std::vector<float> hq = q->hq.empty() ? design::firhilb_taps(q->m, 60.0f) : q->hq;
            std::copy(hq.begin(), hq.end(), hilbert);
        }
    });
}
// A walker whose wait for the previous call's state timed out has walked from a
// stale state: its call's output is invalid.  Raised at every entry point of the
// object (and after the host path's synchronisation) until ldsp_ampmodem_reset.
static void amp_check_err(const AmpObj* q)
{
    const bool dev_flag = q->herr && __atomic_load_n(q->herr, __ATOMIC_ACQUIRE) != 0;
    if (q->st.werr || dev_flag)
        throw Error(LDSP_EHIP, "ampmodem: a PLL walker's wait for the previous call's state timed out; "
                               "the output of that call is not valid (reset the object)");
}
int ldsp_ampmodem_get_pll_state(ldsp_ampmodem_t q, uint32_t* t, uint32_t* d)
{
    return guard([&] {
        NONNULL(q);
        if (q->dev_newer) {
            DeviceGuard g(q->device);
            q->sync_all();
            LDSP_HIP(hipMemcpy(&q->st, q->dst.p, sizeof(q->st), hipMemcpyDeviceToHost));
            q->dev_newer = false;
            amp_check_err(q);
        }
        if (t) *t = q->st.theta;
        if (d) *d = q->st.dtheta;
    });
}

int ldsp_debug_walk_early(int on)
{
    return g_walk_early.exchange(on < 0 ? -1 : (on != 0));
}

int ldsp_debug_iir_sect_trace(void* dev_buf)
{
    return k::iir_sect_trace(dev_buf);
}

int ldsp_debug_pll_margin(int log2_b)
{
    return k::pll_margin_override(log2_b);
}

int ldsp_debug_walk_fold(uint32_t u, int32_t b, int left_gap, int right_gap, uint32_t dk2, uint32_t out[4])
{
    if (!out || u >= (1u << 22) || b < 1 || b > (1 << 21)) return LDSP_EINVAL;
    const k::WalkFold f = k::pll_walk_fold(u, b, left_gap != 0, right_gap != 0, dk2);
    out[0] = (uint32_t)f.lo;
    out[1] = f.W;
    out[2] = f.amin;
    out[3] = f.awidth;
    return LDSP_OK;
}

int ldsp_ampmodem_walk_stats(ldsp_ampmodem_t q, uint64_t* entries, uint64_t* repairs, uint64_t* fallbacks)
{
    return guard([&] {
        NONNULL(q);
        unsigned long long stt[5] = {0, 0, 0, 0, 0};
        if (q->last_stats) {
            DeviceGuard g(q->device);
            q->sync_all();
            LDSP_HIP(hipMemcpy(stt, q->last_stats, sizeof(stt), hipMemcpyDeviceToHost));
        }
        if (entries) *entries = stt[4];
        if (repairs) *repairs = stt[0];
        if (fallbacks) *fallbacks = stt[1];
    });
}

int ldsp_ampmodem_walk_active(ldsp_ampmodem_t q, uint64_t* ticks, uint64_t* count)
{
    return guard([&] {
        NONNULL(q);
        k::AmpState st{};
        if (q->dst.p) {
            DeviceGuard g(q->device);
            q->sync_all();
            LDSP_HIP(hipMemcpy(&st, q->dst.p, sizeof(st), hipMemcpyDeviceToHost));
            q->st.werr = st.werr;
            amp_check_err(q);
        }
        if (ticks) *ticks = st.wact;
        if (count) *count = st.wact_n;
    });
}
int ldsp_ampmodem_walk_clocks(ldsp_ampmodem_t q, uint64_t* walk, uint64_t* wait)
{
    return guard([&] {
        NONNULL(q);
        unsigned long long stt[4] = {0, 0, 0, 0};
        if (q->last_stats) {
            DeviceGuard g(q->device);
            q->sync_all();
            LDSP_HIP(hipMemcpy(stt, q->last_stats, sizeof(stt), hipMemcpyDeviceToHost));
        }
        if (walk) *walk = stt[2];
        if (wait) *wait = stt[3];
    });
}

int ldsp_ampmodem_seq_stats(ldsp_ampmodem_t q, uint64_t* batches, uint64_t* redone)
{
    return guard([&] {
        NONNULL(q);
        k::AmpState st{};
        if (q->dst.p) {
            DeviceGuard g(q->device);
            q->sync_all();
            LDSP_HIP(hipMemcpy(&st, q->dst.p, sizeof(st), hipMemcpyDeviceToHost));
        }
        if (batches) *batches = st.sq_batches;
        if (redone) *redone = st.sq_redone;
    });
}

// Carrier lowpass + delay + PLL walk of AmpModem / BroadcastAM: writes
// re(v1) / mod_index (costas 0) or the Costas-loop output (costas 1) to mbuf
// (slot scratch when mbuf is null).  Returns the buffer written.  The caller
// enqueues its post-filter and then amp_call_end().  Stream order (see AmpObj):
//   wait slot[s] (call k-2 done with slot s) and front (call k-1's histories and guess)
//   lowpass, delay history, candidates            -> mark front
//   wait ord (call k-1's walk; ord is marked before its DC blocker) -> walker
// Costas: the candidates start from the true state (the loop's two stable
// points half a turn apart make a guess ambiguous), so its front also waits for
// call k-1's walk.
// Calls above kAmpPieceMax samples run as consecutive sub-calls of at most that
// many (same bits: every stage streams its state across calls): the walker stores
// repaired outputs through 32-bit byte offsets (k_pll.hip), so one launch covers < 2^30.
static constexpr size_t kAmpPieceMax = size_t(1) << 29;

static float* amp_pll_stage(AmpObj* q, const Exec& e, const void* dx, size_t n, float mod_index, int costas, float* mbuf,
                            int out_idx = 0)
{
    const int L = 2 * (int)q->m + 1;
    const int sl = (int)(q->ncall & 1);
    const int h3 = (int)(q->ncall % 3);
    q->slot[sl].wait(e.stream);
    q->front.wait(e.stream);
    if (costas) q->ord.wait(e.stream);
    if (!mbuf) mbuf = (float*)q->mb[sl].ensure(n * 4, q->device);
    void* x0 = q->x0[sl].ensure(n * 8, q->device);
    k::fir_exact(true, dx, q->lph.in(), q->lph.out(), n, q->dlp.as<float>(), L, 1.0f, x0, e.stream);
    k::PllCall c;
    c.x0 = x0;
    c.x = dx;
    c.hist = q->dlh[h3].p;
    c.hist_out = q->dlh[(h3 + 1) % 3].p;
    c.m = (int)q->m;
    c.n = n;
    c.st = q->dst.as<k::AmpState>();
    c.gcur = (int)(q->ncall & 1);
    c.table = q->dtab.as<float>();
    c.mod_index = mod_index;
    c.costas = costas;
    c.out_idx = out_idx;
    c.alpha_host = q->st.alpha;
    c.y = mbuf;
    c.scratch = k::pll_parallel(n, costas) ? q->pll[sl].ensure(k::pll_scratch_bytes(n), q->device) : nullptr;
    c.wexp = q->wexp;
    q->last_stats = c.scratch ? (const char*)c.scratch + k::pll_stats_offset(n) : nullptr;
    k::pll_front(c, e.stream);
    const bool par = k::pll_parallel(n, costas);
    if (par) q->front.mark(e.stream);     // the sequential loop writes the guess itself: mark after it
    // (A dedicated high-priority walker queue was measured: the ~25 us between
    // walks stayed -- it is the dispatcher waiting for a whole CU to drain for the
    // walker's 135 KiB of LDS, not the cross-queue event -- and the chain slowed.)
    // Early hand-off: the carrier walker does not wait for the previous call's
    // walk on the stream; it is dispatched as soon as its candidates are ready and
    // waits on the device for the state's epoch (k_pll_walk_body), so the CU it
    // needs is taken while the previous walk still runs.  The sequential loops and
    // Costas keep the stream order.
    static const bool early_knob = LDSP_KNOB("LDSP_WALK_EARLY", 1) != 0;
    const int ov = g_walk_early.load(std::memory_order_relaxed);
    const bool early_on = ov < 0 ? early_knob : ov != 0;
    // (calls up to 2^26 samples, after one of at most that: the previous walk then
    // takes < 0.1 s, far inside the walker's 1 s bound on its wait)
    const bool early = early_on && par && !costas && q->live.early_ok() &&
                       n <= (size_t(1) << 26) && q->last_pll_n <= (size_t(1) << 26);
    if (!early) q->ord.wait(e.stream);
    k::pll_back(c, e.stream);
    if (n > 0) {
        q->wexp++;
        q->last_pll_n = n;
    }
    q->ord.mark(e.stream);                // the true PLL state: the next call's walk may start
    if (!par) q->front.mark(e.stream);
    static const bool dbg_pll = LDSP_KNOB("LDSP_DEBUG_PLL", 0) != 0;
    if (par && dbg_pll) {
        unsigned long long stt[7];
        LDSP_HIP(hipMemcpyAsync(stt, (char*)c.scratch + k::pll_stats_offset(n), sizeof(stt), hipMemcpyDeviceToHost,
                                e.stream));
        LDSP_HIP(hipStreamSynchronize(e.stream));
        std::fprintf(stderr, "[ldsp pll] n=%zu entries=%llu repairs=%llu fallback_lane_blocks=%llu walk_clk=%llu "
                     "wait_clk=%llu lane_blocks_repaired=%llu first_pass_set_final=%llu\n", n, stt[4], stt[0], stt[1],
                     stt[2], stt[3], stt[5], stt[6]);
    }
    return mbuf;
}

static void amp_call_end(AmpObj* q, const Exec& e)
{
    q->slot[q->ncall & 1].mark(e.stream);
    q->ncall++;
    q->lph.flip();
    q->dch.flip();
    q->dev_newer = true;
}

// usb / lsb (liquid ampmodem_demod_ssb_pll_carrier / ampmodem_demod_ssb, see
// oracle/liquid_restate.c).  Carrier: the DSB carrier PLL stage writes each
// sample's table index, k_ssb_v1 recomputes v1 = delay(x) mixed down by it, the
// Hilbert c2r keeps the sideband (0.5 * . / mod_index) and the DC blocker
// follows.  Suppressed carrier: the Hilbert c2r of x alone.  The Hilbert history
// is ordered across streams by `post` (like the DC blocker's).
static void amp_ssb(AmpObj* q, const Exec& e, const void* dx, size_t n, float* dy)
{
    const int M = (int)q->m, H = 4 * M - 1, usb = q->type == 1 ? 1 : 0;
    if (q->suppressed) {
        q->post.wait(e.stream);
        k::ssb_c2r(dx, q->hbh.in(), n, q->dhq.as<float>(), M, usb, q->mod_index, dy, e.stream);
        k::delay_hist(dx, q->hbh.in(), q->hbh.out(), n, H, e.stream);
        q->post.mark(e.stream);
        q->hbh.flip();
        return;
    }
    const int L = 2 * M + 1;
    const int sl = (int)(q->ncall & 1);
    const void* dhist = q->dlh[q->ncall % 3].p;           // this call's delay-line history (read by the PLL stage too)
    float* mbuf = amp_pll_stage(q, e, dx, n, q->mod_index, 0, nullptr, 1);
    void* v1 = q->v1[sl].ensure(n * 8, q->device);
    q->post.wait(e.stream);
    k::ssb_v1(mbuf, dx, dhist, M, q->dtab.as<float>(), n, v1, e.stream);
    k::ssb_c2r(v1, q->hbh.in(), n, q->dhq.as<float>(), M, usb, q->mod_index, mbuf, e.stream);
    k::delay_hist(v1, q->hbh.in(), q->hbh.out(), n, H, e.stream);
    k::fir_exact(false, mbuf, q->dch.in(), q->dch.out(), n, q->ddc.as<float>(), L, 1.0f, dy, e.stream);
    q->post.mark(e.stream);
    q->hbh.flip();
    amp_call_end(q, e);
}

int ldsp_ampmodem_demodulate(ldsp_ampmodem_t q, const void* x, size_t n, void* y, int mem, void* stream)
{
    LDSP_RANGE("ldsp_ampmodem_demodulate");
    return guard([&] {
        NONNULL(q);
        LDSP_REQUIRE(n == 0 || (x && y), "ampmodem_demodulate: NULL buffer");
        if (n > kAmpPieceMax) {              // the walker's 32-bit store offsets: consecutive sub-calls
            for (size_t off = 0; off < n; off += kAmpPieceMax) {
                ok(ldsp_ampmodem_demodulate(q, (const char*)x + off * 8, std::min(kAmpPieceMax, n - off),
                                            (char*)y + off * 4, mem, stream));
            }
            return;
        }
        amp_check_err(q);
        Call call(*q, mem, x, stream, false);     // the PLL stage orders its parts itself: amp_pll_stage, amp_call_end
        const Exec& e = call.e;
        const void* dx = q->stg.dev_in(e, x, n * 8);
        float* dy = (float*)q->stg.dev_out(e, y, n * 4);
        if (n > 0 && q->type != 0) {
            amp_ssb(q, e, dx, n, dy);
        } else if (n > 0) {
            const int L = 2 * (int)q->m + 1;
            float* mbuf = amp_pll_stage(q, e, dx, n, q->mod_index, q->suppressed ? 1 : 0, q->suppressed ? dy : nullptr);
            if (!q->suppressed) {
                // the DC blocker is off the walker's chain: the next call's walk
                // waits for this walk only (ord), the next DC blocker for this one
                q->post.wait(e.stream);
                k::fir_exact(false, mbuf, q->dch.in(), q->dch.out(), n, q->ddc.as<float>(), L, 1.0f, dy, e.stream);
                q->post.mark(e.stream);
            }
            amp_call_end(q, e);
        }
        call.end();
        q->stg.finish(e, y, n * 4);
        if (e.host) amp_check_err(q);         // synchronised: this call's own walk is done
    });
}

int ldsp_debug_ampmodem_dispatch(ldsp_ampmodem_t q, size_t n, int* parallel, int* batchable)
{
    return guard([&] {
        NONNULL(q);
        if (parallel) *parallel = k::pll_parallel(n, q->suppressed ? 1 : 0) ? 1 : 0;
        if (batchable) *batchable = q->type == 0 ? 1 : 0;
    });
}
int ldsp_debug_ampmodem_handoff(ldsp_ampmodem_t q, uint64_t wait_ticks, int epoch_skew)
{
    return guard([&] {
        NONNULL(q);
        DeviceGuard g(DevObj::bind_first(*q, current_device()));
        q->sync_all();
        q->st.wait_ticks = wait_ticks ? (unsigned long long)wait_ticks : kWalkWaitTicks;
        LDSP_HIP(hipMemcpy((char*)q->dst.p + offsetof(k::AmpState, wait_ticks), &q->st.wait_ticks,
                           sizeof(q->st.wait_ticks), hipMemcpyHostToDevice));
        q->wexp += (uint32_t)epoch_skew;
    });
}

// ---------------------------------------------------------------- BroadcastAM
int ldsp_bcastam_create(unsigned int m, ldsp_bcastam_t* q)
{
    return guard([&] {
        NONNULL(q);
        LDSP_REQUIRE(m >= 1 && m <= 4096, "bcastam: m must be in [1, 4096]");
        std::unique_ptr<ldsp_bcastam_s> o(new ldsp_bcastam_s());
        o->mod_index = 1.0f;
        o->type = 0;
        o->suppressed = 0;
        o->m = m;
        o->lp = design::firdes_kaiser(2 * m + 1, 0.01f, 40.0f, 0.0f);
        o->table = nco_table();
        o->reset_host();
        // cheby2 highpass, SOS, order 3, fc 20/48000, f0 0, Ap 0.5, As 20 (demod.hpp:104)
        ok(ldsp_iirfilt_create_prototype(2, 1, 3, 20.0f / 48000.0f, 0.0f, 0.5f, 20.0f, 0, &o->dcb));
        *q = o.release();
    });
}
int ldsp_bcastam_destroy(ldsp_bcastam_t q) { return guard([&] { destroy(q); }); }   // and its DC blocker
int ldsp_bcastam_reset(ldsp_bcastam_t q)
{
    return guard([&] {
        NONNULL(q);
        amp_reset(q);
        ok(ldsp_iirfilt_reset(q->dcb));
    });
}
int ldsp_bcastam_set_mode(ldsp_bcastam_t q, int mode)
{
    return guard([&] {
        NONNULL(q);
        ok(ldsp_iirfilt_set_mode(q->dcb, mode));
    });
}
int ldsp_bcastam_get_mode(ldsp_bcastam_t q, int* mode)
{
    return guard([&] {
        NONNULL(q);
        NONNULL(mode);
        *mode = q->dcb->mode;
    });
}
int ldsp_bcastam_demodulate(ldsp_bcastam_t q, const void* x, size_t n, void* y, void* pre, int mem, void* stream)
{
    LDSP_RANGE("ldsp_bcastam_demodulate");
    return guard([&] {
        NONNULL(q);
        LDSP_REQUIRE(n == 0 || (x && y), "bcastam_demodulate: NULL buffer");
        if (n > kAmpPieceMax) {              // as ldsp_ampmodem_demodulate
            for (size_t off = 0; off < n; off += kAmpPieceMax) {
                const size_t m = std::min(kAmpPieceMax, n - off);
                ok(ldsp_bcastam_demodulate(q, (const char*)x + off * 8, m, (char*)y + off * 4,
                                           pre ? (char*)pre + off * 4 : nullptr, mem, stream));
            }
            return;
        }
        amp_check_err(q);
        Call call(*q, mem, x, stream, false);     // as ldsp_ampmodem_demodulate
        const Exec& e = call.e;
        const void* dx = q->stg.dev_in(e, x, n * 8);
        float* dy = (float*)q->stg.dev_out(e, y, n * 4);
        if (n > 0) {
            float* mbuf = amp_pll_stage(q, e, dx, n, 1.0f, 0, nullptr);
            ok(ldsp_iirfilt_execute(q->dcb, mbuf, n, dy, LDSP_MEM_DEVICE, e.stream));
            if (pre) {
                LDSP_HIP(hipMemcpyAsync(pre, mbuf, n * 4, e.host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice,
                                        e.stream));
            }
            amp_call_end(q, e);
        }
        call.end();
        q->stg.finish(e, y, n * 4);
        if (e.host) amp_check_err(q);
    });
}

// ---------------------------------------------------------------- FreqDem
int ldsp_freqdem_create(float kf, ldsp_freqdem_t* q)
{
    return guard([&] {
        NONNULL(q);
        LDSP_REQUIRE(kf > 0.0f, "freqdem: kf must be > 0");
        std::unique_ptr<ldsp_freqdem_s> o(new ldsp_freqdem_s());
        o->kf = kf;
        o->ref = (float)(1.0 / (2 * M_PI * (double)kf));   // freqdem.c: 1/(2*M_PI*kf) in double, stored float
        *q = o.release();
    });
}
int ldsp_freqdem_destroy(ldsp_freqdem_t q) { return guard([&] { destroy(q); }); }
int ldsp_freqdem_reset(ldsp_freqdem_t q)
{
    return guard([&] {
        NONNULL(q);
        q->at_rest([&] { q->prev.zero(8, q->device); });
    });
}
int ldsp_freqdem_get_kf(ldsp_freqdem_t q, float* kf)
{
    return guard([&] {
        NONNULL(q);
        NONNULL(kf);
        *kf = q->kf;
    });
}
int ldsp_freqdem_demodulate(ldsp_freqdem_t q, const void* x, size_t n, void* y, int mem, void* stream)
{
    LDSP_RANGE("ldsp_freqdem_demodulate");
    return guard([&] {
        NONNULL(q);
        LDSP_REQUIRE(n == 0 || (x && y), "freqdem_demodulate: NULL buffer");
        Call call(*q, mem, x, stream);
        const Exec& e = call.e;
        const void* dx = q->stg.dev_in(e, x, n * 8);
        float* dy = (float*)q->stg.dev_out(e, y, n * 4);
        if (n > 0) {
            k::freqdem(dx, q->prev.in(), q->prev.out(), n, q->ref, dy, e.stream);
            q->prev.flip();
        }
        call.end();
        q->stg.finish(e, y, n * 4);
    });
}

// ---------------------------------------------------------------- Delay
int ldsp_delay_create(unsigned int nd, ldsp_delay_t* q)
{
    return guard([&] {
        NONNULL(q);
        LDSP_REQUIRE(nd <= (1u << 26), "delay: nd too large");
        std::unique_ptr<ldsp_delay_s> o(new ldsp_delay_s());
        o->nd = nd;
        *q = o.release();
    });
}
int ldsp_delay_destroy(ldsp_delay_t q) { return guard([&] { destroy(q); }); }
int ldsp_delay_set_delay(ldsp_delay_t q, unsigned int nd)
{
    return guard([&] {
        NONNULL(q);
        LDSP_REQUIRE(nd <= (1u << 26), "delay: nd too large");
        q->nd = nd;
        q->at_rest([&] { q->zero(q->device); });
    });
}
int ldsp_delay_get_delay(ldsp_delay_t q, unsigned int* nd)
{
    return guard([&] {
        NONNULL(q);
        NONNULL(nd);
        *nd = q->nd;
    });
}
int ldsp_delay_execute(ldsp_delay_t q, const void* x, size_t n, int cplx, void* y, int mem, void* stream)
{
    LDSP_RANGE("ldsp_delay_execute");
    return guard([&] {
        NONNULL(q);
        LDSP_REQUIRE(n == 0 || (x && y), "delay_execute: NULL buffer");
        Call call(*q, mem, x, stream);
        const Exec& e = call.e;
        const size_t es = cplx ? 8 : 4;
        const void* dx = q->stg.dev_in(e, x, n * es);
        void* dy = q->stg.dev_out(e, y, n * es);
        if (n > 0) {
            const int D = (int)q->nd + 1;
            PingPong& h = cplx ? q->hc : q->hr;
            k::delay(cplx != 0, dx, h.in(), h.out(), n, D, dy, e.stream);
            h.flip();
        }
        call.end();
        q->stg.finish(e, y, n * es);
    });
}

// ---------------------------------------------------------------- firhilbf
static_assert(LDSP_HILB_R2C == k::kHilbR2C && LDSP_HILB_C2R == k::kHilbC2R && LDSP_HILB_DECIM == k::kHilbDecim &&
                  LDSP_HILB_INTERP == k::kHilbInterp,
              "ldsp.h and kernels.hpp number the Hilbert operations alike");
int ldsp_firhilb_create(unsigned int m, float as, int op, ldsp_firhilb_t* q)
{
    return guard([&] {
        NONNULL(q);
        LDSP_REQUIRE(m >= 2, "firhilb: filter semi-length must be at least 2");
        LDSP_REQUIRE(op == LDSP_HILB_R2C || op == LDSP_HILB_C2R || op == LDSP_HILB_DECIM || op == LDSP_HILB_INTERP,
                     "firhilb: op must be one of LDSP_HILB_R2C, _C2R, _DECIM, _INTERP");
        if (m > (unsigned)k::kHilbMaxM)
            throw Error(LDSP_EUNSUP, "firhilb: semi-length above " + std::to_string(k::kHilbMaxM) + " is not implemented");
        std::unique_ptr<ldsp_firhilb_s> o(new ldsp_firhilb_s());
        o->m = m;
        o->op = op;
        o->hq = design::firhilb_taps(m, as);
        *q = o.release();
    });
}
int ldsp_firhilb_destroy(ldsp_firhilb_t q) { return guard([&] { destroy(q); }); }
int ldsp_firhilb_reset(ldsp_firhilb_t q)
{
    return guard([&] {
        NONNULL(q);
        q->at_rest([&] { q->hist.zero(q->hist_bytes(), q->device); });
    });
}
int ldsp_firhilb_get_taps(ldsp_firhilb_t q, float* hq)
{
    return guard([&] {
        NONNULL(q);
        NONNULL(hq);
        std::copy(q->hq.begin(), q->hq.end(), hq);
    });
}
int ldsp_firhilb_execute(ldsp_firhilb_t q, const void* x, size_t n, void* y0, void* y1, int mem, void* stream)
{
    LDSP_RANGE("ldsp_firhilb_execute");
    return guard([&] {
        NONNULL(q);
        const int op = q->op;
        if (op == LDSP_HILB_C2R) LDSP_REQUIRE(y0 || y1, "firhilb_execute: c2r needs y0 (lower) or y1 (upper)");
        else LDSP_REQUIRE(!y1, "firhilb_execute: y1 must be NULL unless the object is c2r");
        LDSP_REQUIRE(op != LDSP_HILB_DECIM || n % 2 == 0, "firhilb_execute: decim takes an even number of samples");
        LDSP_REQUIRE(n == 0 || (x && (y0 || op == LDSP_HILB_C2R)), "firhilb_execute: NULL buffer");
        Call call(*q, mem, x, stream);
        const Exec& e = call.e;
        // output samples and their size
        const size_t no = op == LDSP_HILB_DECIM ? n / 2 : (op == LDSP_HILB_INTERP ? 2 * n : n);
        const size_t os = op == LDSP_HILB_R2C || op == LDSP_HILB_DECIM ? 8 : 4;
        const void* dx = q->stg.dev_in(e, x, n * q->in_size());
        void* d0 = y0 ? q->stg.dev_out(e, y0, no * os) : nullptr;
        void* d1 = y1 ? q->stg1.dev_out(e, y1, no * os) : nullptr;
        if (n > 0) {
            k::hilbert(op, dx, q->hist.in(), q->hist.out(), n, q->dhq.as<float>(), (int)q->m, d0, d1, e.stream);
            q->hist.flip();
        }
        call.end();
        if (y0) q->stg.finish(e, y0, no * os);
        if (y1) q->stg1.finish(e, y1, no * os);
    });
}
int ldsp_debug_firhilb_tile(int op, size_t* samples)
{
    return guard([&] {
        NONNULL(samples);
        LDSP_REQUIRE(op >= LDSP_HILB_R2C && op <= LDSP_HILB_INTERP, "firhilb: unknown op");
        *samples = op == LDSP_HILB_INTERP ? k::kHilbTile / 2 : k::kHilbTile;
    });
}

// ---------------------------------------------------------------- Channelizer, Synthesizer
// What the two banks' entry points do alike takes the words that differ from here.
struct BankKind {
    const char* pre;                  // the messages' prefix
    const char* rate;                 // what D is
    const char* taps;                 // the taps argument's name
    bool synth;
};
static const BankKind kChan{"chan", "decimation", "h", false}, kSynth{"synth", "interpolation", "g", true};

static void bank_check_channels(const BankKind& kind, unsigned int M)
{
    if (M > 256) throw Error(LDSP_EUNSUP, std::string(kind.pre) + ": more than 256 channels is not implemented");
}
static void bank_check_shape(const BankKind& kind, unsigned int M, unsigned int D)
{
    LDSP_REQUIRE(M >= 4 && (M & (M - 1)) == 0,
                 std::string(kind.pre) + ": the channel count must be a power of two, at least 4");
    LDSP_REQUIRE(D == M || 2 * D == M, std::string(kind.pre) + ": the " + kind.rate +
                                           " must be M (critically sampled) or M / 2 (2x oversampled)");
}
extern "C++" {
template <class T>
static T* bank_make(const BankKind& kind, unsigned int M, unsigned int D, std::vector<float> h, float scale)
{
    bank_check_channels(kind, M);
    if (h.size() > (size_t)k::kChanMaxP * M)
        throw Error(LDSP_EUNSUP, std::string(kind.pre) + ": more than " + std::to_string(k::kChanMaxP) +
                                     " taps per branch (L > " + std::to_string(k::kChanMaxP) + " M) is not implemented");
    std::unique_ptr<T> o(new T());
    o->M = M;
    o->D = D;
    o->R = (unsigned)((h.size() + (kind.synth ? D : M) - 1) / (kind.synth ? D : M));
    o->hist_bytes = (kind.synth ? std::max<size_t>((size_t)M * (o->R - 1), 1) : (size_t)o->R * M - 1) * 8;
    o->h = std::move(h);
    o->scale = scale;
    return o.release();
}
template <class T>
static int bank_create_taps(const BankKind& kind, unsigned int M, unsigned int D, const float* h, unsigned int L, T** q)
{
    return guard([&] {
        NONNULL(q);
        bank_check_shape(kind, M, D);
        LDSP_REQUIRE(L >= 1, std::string(kind.pre) + ": at least one tap");
        LDSP_REQUIRE(h != nullptr, std::string(kind.taps) + " must not be NULL");
        *q = bank_make<T>(kind, M, D, std::vector<float>(h, h + L), 1.0f);
    });
}
} // extern "C++"
// The Kaiser prototype of 2 M m + 1 taps and their sum in double; a cutoff that
// is not positive stands for the bank's default `fc0`.
static std::vector<float> bank_prototype(const BankKind& kind, unsigned int M, unsigned int m, float fc, float fc0,
                                         float as, double* sum)
{
    const std::string pre(kind.pre);
    LDSP_REQUIRE(m >= 1, pre + ": filter semi-length must be at least 1");
    LDSP_REQUIRE(as > 0.0f, pre + ": stop-band attenuation must be > 0");
    LDSP_REQUIRE(fc < 0.5f, pre + ": cutoff must be below 0.5");
    bank_check_channels(kind, M);
    if (2 * (size_t)m + 1 > (size_t)k::kChanMaxP)
        throw Error(LDSP_EUNSUP, pre + ": semi-length above " + std::to_string((k::kChanMaxP - 1) / 2) +
                                     " is not implemented");
    std::vector<float> h = design::firdes_kaiser(2 * M * m + 1, fc > 0.0f ? fc : fc0, as, 0.0f);
    *sum = 0.0;
    for (float v : h) *sum += (double)v;
    return h;
}
static int bank_reset(BankObj* q)
{
    return guard([&] {
        NONNULL(q);
        q->seen = 0;
        q->at_rest([&] { q->hist.zero(q->hist_bytes, q->device); });
    });
}
static int bank_get_taps(const BankKind& kind, const BankObj* q, float* h)
{
    return guard([&] {
        NONNULL(q);
        LDSP_REQUIRE(h != nullptr, std::string(kind.taps) + " must not be NULL");
        std::copy(q->h.begin(), q->h.end(), h);
    });
}
static int bank_get_scale(const BankObj* q, float* s) { return guard([&] { NONNULL(q); NONNULL(s); *s = q->scale; }); }
static int bank_set_scale(BankObj* q, float s) { return guard([&] { NONNULL(q); q->scale = s; }); }

int ldsp_chan_create(unsigned int M, unsigned int D, unsigned int m, float fc, float as, ldsp_chan_t* q)
{
    return guard([&] {
        NONNULL(q);
        bank_check_shape(kChan, M, D);
        double sum = 0.0;
        std::vector<float> h = bank_prototype(kChan, M, m, fc, 0.5f / (float)M, as, &sum);
        *q = bank_make<ldsp_chan_s>(kChan, M, D, std::move(h), (float)(1.0 / sum));
    });
}
int ldsp_chan_create_taps(unsigned int M, unsigned int D, const float* h, unsigned int L, ldsp_chan_t* q)
{
    return bank_create_taps(kChan, M, D, h, L, q);
}
int ldsp_chan_destroy(ldsp_chan_t q) { return guard([&] { destroy(q); }); }
int ldsp_chan_reset(ldsp_chan_t q) { return bank_reset(q); }
int ldsp_chan_get_info(ldsp_chan_t q, unsigned int* M, unsigned int* D, unsigned int* L, unsigned int* skip)
{
    return guard([&] {
        NONNULL(q);
        if (M) *M = q->M;
        if (D) *D = q->D;
        if (L) *L = (unsigned)q->h.size();
        if (skip) *skip = (unsigned)q->skip();
    });
}
int ldsp_chan_get_taps(ldsp_chan_t q, float* h) { return bank_get_taps(kChan, q, h); }
int ldsp_chan_get_scale(ldsp_chan_t q, float* s) { return bank_get_scale(q, s); }
int ldsp_chan_set_scale(ldsp_chan_t q, float s) { return bank_set_scale(q, s); }
int ldsp_chan_num_outputs(ldsp_chan_t q, size_t n, size_t* ncols)
{
    return guard([&] {
        NONNULL(q);
        NONNULL(ncols);
        *ncols = q->num_outputs(n);
    });
}
// iq16: x is n int16 (I, Q) pairs (bytes_to_iq's input), converted by the kernel's loads
static int chan_execute(ldsp_chan_t q, const void* x, size_t n, void* y, size_t ld, size_t* ncols, int mem, void* stream,
                        bool iq16)
{
    return guard([&] {
        NONNULL(q);
        const size_t K = q->num_outputs(n);
        if (ncols) *ncols = K;
        if (K > ld) throw Error(LDSP_ERANGE, "chan_execute: row stride below the number of output columns");
        LDSP_REQUIRE(n == 0 || x, "chan_execute: NULL input");
        LDSP_REQUIRE(K == 0 || y, "chan_execute: NULL output");
        Call call(*q, mem, x, stream);
        const Exec& e = call.e;
        const unsigned M = q->M, D = q->D;
        // a host-memory call computes into a dense [M][K] device image
        // (rows of the caller's image are ld samples apart)
        const size_t dld = e.host ? K : ld;
        const void* dx = q->stg.dev_in(e, x, n * (iq16 ? 4 : 8));
        void* dy = q->stg.dev_out(e, y, (size_t)M * K * 8);
        if (n > 0) {
            k::ChanCall c;
            c.x = dx;
            c.hist = q->hist.in();
            c.hist_out = q->hist.out();
            c.n = n;
            c.skip = q->skip();
            c.ncols = K;
            c.ld = dld;
            c.parity = q->parity();
            c.P = (int)q->R;
            c.taps = q->dtaps.as<float>();
            c.tw = q->dtw.p;
            c.scale = q->scale;
            c.y = dy;
            c.iq16 = iq16;
            k::chan((int)M, (int)D, c, e.stream);
            q->hist.flip();
            q->seen += n;
        }
        call.end();
        q->stg.finish(e, y, K * 8, M, ld * 8);
    });
}
int ldsp_chan_execute(ldsp_chan_t q, const void* x, size_t n, void* y, size_t ld, size_t* ncols, int mem, void* stream)
{
    LDSP_RANGE("ldsp_chan_execute");
    return chan_execute(q, x, n, y, ld, ncols, mem, stream, false);
}
int ldsp_chan_execute_iq16(ldsp_chan_t q, const void* x, size_t n, void* y, size_t ld, size_t* ncols, int mem,
                           void* stream)
{
    LDSP_RANGE("ldsp_chan_execute_iq16");
    return chan_execute(q, x, n, y, ld, ncols, mem, stream, true);
}
int ldsp_debug_chan_tile(unsigned int M, unsigned int D, size_t* frames)
{
    return guard([&] {
        NONNULL(frames);
        bank_check_shape(kChan, M, D);
        bank_check_channels(kChan, M);
        *frames = (size_t)k::chan_frames((int)M);
    });
}

int ldsp_synth_create(unsigned int M, unsigned int D, unsigned int m, float fc, float as, ldsp_synth_t* q)
{
    return guard([&] {
        NONNULL(q);
        bank_check_shape(kSynth, M, D);
        // D = M / 2: flat across the analysis prototype's transition band, stopped before the image at 2 / M
        double sum = 0.0;
        std::vector<float> g = bank_prototype(kSynth, M, m, fc, (D == M ? 0.5f : 1.0f) / (float)M, as, &sum);
        *q = bank_make<ldsp_synth_s>(kSynth, M, D, std::move(g), (float)((double)D / sum));
    });
}
int ldsp_synth_create_taps(unsigned int M, unsigned int D, const float* g, unsigned int L, ldsp_synth_t* q)
{
    return bank_create_taps(kSynth, M, D, g, L, q);
}
int ldsp_synth_destroy(ldsp_synth_t q) { return guard([&] { destroy(q); }); }
int ldsp_synth_reset(ldsp_synth_t q) { return bank_reset(q); }
int ldsp_synth_get_info(ldsp_synth_t q, unsigned int* M, unsigned int* D, unsigned int* L)
{
    return guard([&] {
        NONNULL(q);
        if (M) *M = q->M;
        if (D) *D = q->D;
        if (L) *L = (unsigned)q->h.size();
    });
}
int ldsp_synth_get_taps(ldsp_synth_t q, float* g) { return bank_get_taps(kSynth, q, g); }
int ldsp_synth_get_scale(ldsp_synth_t q, float* s) { return bank_get_scale(q, s); }
int ldsp_synth_set_scale(ldsp_synth_t q, float s) { return bank_set_scale(q, s); }
int ldsp_synth_num_outputs(ldsp_synth_t q, size_t ncols, size_t* n)
{
    return guard([&] {
        NONNULL(q);
        NONNULL(n);
        *n = ncols * q->D;
    });
}
int ldsp_synth_execute(ldsp_synth_t q, const void* y, size_t ld, size_t ncols, void* z, size_t cap, size_t* n, int mem,
                       void* stream)
{
    LDSP_RANGE("ldsp_synth_execute");
    return guard([&] {
        NONNULL(q);
        const unsigned M = q->M, D = q->D;
        const size_t K = ncols, N = K * D;
        if (n) *n = N;
        LDSP_REQUIRE(ld >= K, "synth_execute: row stride below the number of columns");
        if (cap < N) throw Error(LDSP_ERANGE, "synth_execute: output capacity below ncols * D");
        LDSP_REQUIRE(K == 0 || y, "synth_execute: NULL input");
        LDSP_REQUIRE(K == 0 || z, "synth_execute: NULL output");
        Call call(*q, mem, y, stream);
        const Exec& e = call.e;
        // a host-memory call reads a dense [M][K] device image
        // (rows of the caller's image are ld samples apart)
        const size_t dld = e.host ? K : ld;
        const void* dy = q->stg.dev_in(e, y, K * 8, M, ld * 8);
        void* dz = q->stg.dev_out(e, z, N * 8);
        if (K > 0) {
            k::SynthCall c;
            c.y = dy;
            c.hist = q->hist.in();
            c.hist_out = q->hist.out();
            c.ncols = K;
            c.ld = dld;
            c.parity = (int)(q->seen & 1);
            c.Q = (int)q->R;
            c.taps = q->dtaps.as<float>();
            c.tw = q->dtw.p;
            c.scale = q->scale;
            c.z = dz;
            k::synth((int)M, (int)D, c, e.stream);
            q->hist.flip();
            q->seen += K;
        }
        call.end();
        q->stg.finish(e, z, N * 8);
    });
}
int ldsp_debug_synth_tile(unsigned int M, unsigned int D, size_t* cols)
{
    return guard([&] {
        NONNULL(cols);
        bank_check_shape(kSynth, M, D);
        bank_check_channels(kSynth, M);
        *cols = (size_t)k::synth_cols((int)M);
    });
}

// ---------------------------------------------------------------- Downconverter
// w = rint(f 2^32) mod 2^32: the product is exact (a power of two), rint rounds ties to even
static std::vector<uint32_t> ddc_words(const double* f, unsigned int C)
{
    LDSP_REQUIRE(C >= 1, "ddc: at least one tuner");
    if (C > (unsigned)k::kDdcMaxC)
        throw Error(LDSP_EUNSUP, "ddc: more than " + std::to_string(k::kDdcMaxC) + " tuners is not implemented");
    LDSP_REQUIRE(f != nullptr, "f must not be NULL");
    std::vector<uint32_t> w(C);
    for (unsigned c = 0; c < C; c++) {
        LDSP_REQUIRE(std::isfinite(f[c]) && std::fabs(f[c]) <= 1.0,
                     "ddc: a frequency must be finite and at most 1 cycle per sample in magnitude");
        w[c] = (uint32_t)(uint64_t)(int64_t)std::nearbyint(f[c] * 4294967296.0);
    }
    return w;
}
static void ddc_check_decim(unsigned int D)
{
    LDSP_REQUIRE(D >= 1, "ddc: the decimation must be at least 2");
    if (D == 1) throw Error(LDSP_EUNSUP, "ddc: decimation 1 is not implemented (mix_down_filter serves it)");
    if (D > (unsigned)k::kDdcMaxD)
        throw Error(LDSP_EUNSUP, "ddc: decimation above " + std::to_string(k::kDdcMaxD) + " is not implemented");
}
// The Downconverter's and the FMBank's Kaiser prototype of 2 D m + 1 taps with the scale 1 / their sum (in double);
// a cutoff that is not positive stands for 0.5 / D, `pre` is the messages' prefix.  D = 1 decimates nothing: no taps.
static std::pair<std::vector<float>, float> decim_prototype(const std::string& pre, unsigned D, unsigned m, float fc, float as)
{
    LDSP_REQUIRE(m >= 1, pre + ": filter semi-length must be at least 1");
    LDSP_REQUIRE(as > 0.0f, pre + ": stop-band attenuation must be > 0");
    LDSP_REQUIRE(fc < 0.5f, pre + ": cutoff must be below 0.5");
    if (2 * (size_t)m + 1 > (size_t)k::kChanMaxP)
        throw Error(LDSP_EUNSUP, pre + ": semi-length above " + std::to_string((k::kChanMaxP - 1) / 2) +
                                     " is not implemented");
    if (D == 1) return {{}, 1.0f};
    std::vector<float> h = design::firdes_kaiser(2 * D * m + 1, fc > 0.0f ? fc : 0.5f / (float)D, as, 0.0f);
    double sum = 0.0;
    for (float v : h) sum += (double)v;
    return {std::move(h), (float)(1.0 / sum)};
}
// At most kChanMaxP taps per output phase; `bound`: with the create functions' "(L > 17 D) "
static void decim_check_taps(const std::string& pre, size_t L, unsigned D, bool bound)
{
    const std::string P = std::to_string(k::kChanMaxP), b = bound ? "(L > " + P + " D) " : "";
    if (L > (size_t)k::kChanMaxP * D)
        throw Error(LDSP_EUNSUP, pre + ": more than " + P + " taps per output phase " + b + "is not implemented");
}
static ldsp_ddc_s* ddc_make(std::vector<uint32_t> w, unsigned int D, std::vector<float> h, float scale)
{
    decim_check_taps("ddc", h.size(), D, true);
    std::unique_ptr<ldsp_ddc_s> o(new ldsp_ddc_s());
    o->D = D;
    o->h = std::move(h);
    o->w = std::move(w);
    o->scale = scale;
    return o.release();
}
int ldsp_ddc_create(const double* f, unsigned int C, unsigned int D, unsigned int m, float fc, float as, ldsp_ddc_t* q)
{
    return guard([&] {
        NONNULL(q);
        ddc_check_decim(D);
        std::vector<uint32_t> w = ddc_words(f, C);
        auto p = decim_prototype("ddc", D, m, fc, as);
        *q = ddc_make(std::move(w), D, std::move(p.first), p.second);
    });
}
int ldsp_ddc_create_taps(const double* f, unsigned int C, unsigned int D, const float* h, unsigned int L, ldsp_ddc_t* q)
{
    return guard([&] {
        NONNULL(q);
        ddc_check_decim(D);
        std::vector<uint32_t> w = ddc_words(f, C);
        LDSP_REQUIRE(L >= 1, "ddc: at least one tap");
        NONNULL(h);
        *q = ddc_make(std::move(w), D, std::vector<float>(h, h + L), 1.0f);
    });
}
int ldsp_ddc_destroy(ldsp_ddc_t q) { return guard([&] { destroy(q); }); }
static void ddc_restart(ldsp_ddc_t q, uint64_t T)
{
    q->seen = T;
    q->at_rest([&] { q->hist.zero(q->hist_bytes(), q->device); });
}
int ldsp_ddc_reset(ldsp_ddc_t q) { return guard([&] { NONNULL(q); ddc_restart(q, 0); }); }
int ldsp_debug_ddc_seek(ldsp_ddc_t q, uint64_t T) { return guard([&] { NONNULL(q); ddc_restart(q, T); }); }
int ldsp_ddc_set_frequencies(ldsp_ddc_t q, const double* f, unsigned int C)
{
    return guard([&] {
        NONNULL(q);
        std::vector<uint32_t> w = ddc_words(f, C);
        // the tables change only once the object's earlier calls have finished with them
        std::swap(q->w, w);
        try {
            q->at_rest([&] { q->upload_tables(q->device); });
        } catch (...) {
            std::swap(q->w, w);
            throw;
        }
    });
}
int ldsp_ddc_get_words(ldsp_ddc_t q, uint32_t* w)
{
    return guard([&] {
        NONNULL(q);
        NONNULL(w);
        std::copy(q->w.begin(), q->w.end(), w);
    });
}
int ldsp_ddc_get_info(ldsp_ddc_t q, unsigned int* C, unsigned int* D, unsigned int* L, unsigned int* skip)
{
    return guard([&] {
        NONNULL(q);
        if (C) *C = (unsigned)q->w.size();
        if (D) *D = q->D;
        if (L) *L = (unsigned)q->h.size();
        if (skip) *skip = (unsigned)q->skip();
    });
}
int ldsp_ddc_get_taps(ldsp_ddc_t q, float* h)
{
    return guard([&] {
        NONNULL(q);
        NONNULL(h);
        std::copy(q->h.begin(), q->h.end(), h);
    });
}
int ldsp_ddc_get_scale(ldsp_ddc_t q, float* s) { return guard([&] { NONNULL(q); NONNULL(s); *s = q->scale; }); }
int ldsp_ddc_set_scale(ldsp_ddc_t q, float s) { return guard([&] { NONNULL(q); q->scale = s; }); }
int ldsp_ddc_num_outputs(ldsp_ddc_t q, size_t n, size_t* ncols)
{
    return guard([&] {
        NONNULL(q);
        NONNULL(ncols);
        *ncols = q->num_outputs(n);
    });
}
// iq16: x is n int16 (I, Q) pairs (bytes_to_iq's input), converted by the kernel's loads
static int ddc_execute(ldsp_ddc_t q, const void* x, size_t n, void* y, size_t ld, size_t* ncols, int mem, void* stream,
                       bool iq16)
{
    return guard([&] {
        NONNULL(q);
        const size_t K = q->num_outputs(n);
        if (ncols) *ncols = K;
        if (K > ld) throw Error(LDSP_ERANGE, "ddc_execute: row stride below the number of output columns");
        LDSP_REQUIRE(n == 0 || x, "ddc_execute: NULL input");
        LDSP_REQUIRE(K == 0 || y, "ddc_execute: NULL output");
        Call call(*q, mem, x, stream);
        const Exec& e = call.e;
        const size_t C = q->w.size();
        // a host-memory call computes into a dense [C][K] device image
        // (rows of the caller's image are ld samples apart)
        const size_t dld = e.host ? K : ld;
        const void* dx = q->stg.dev_in(e, x, n * (iq16 ? 4 : 8));
        void* dy = q->stg.dev_out(e, y, C * K * 8);
        if (n > 0) {
            k::DdcCall c;
            c.x = dx;
            c.hist = q->hist.in();
            c.hist_out = q->hist.out();
            c.n = n;
            c.skip = q->skip();
            c.ncols = K;
            c.ld = dld;
            c.col0 = q->next_column();
            c.C = (int)C;
            c.L = (int)q->h.size();
            c.taps = q->dtaps.p;
            c.slots = q->dslots.as<int>();
            c.words = q->dwords.as<uint32_t>();
            c.scale = q->scale;
            c.y = dy;
            c.iq16 = iq16;
            k::ddc((int)q->D, c, e.stream);
            q->hist.flip();
            q->seen += n;
        }
        call.end();
        q->stg.finish(e, y, K * 8, C, ld * 8);
    });
}
int ldsp_ddc_execute(ldsp_ddc_t q, const void* x, size_t n, void* y, size_t ld, size_t* ncols, int mem, void* stream)
{
    LDSP_RANGE("ldsp_ddc_execute");
    return ddc_execute(q, x, n, y, ld, ncols, mem, stream, false);
}
int ldsp_ddc_execute_iq16(ldsp_ddc_t q, const void* x, size_t n, void* y, size_t ld, size_t* ncols, int mem,
                          void* stream)
{
    LDSP_RANGE("ldsp_ddc_execute_iq16");
    return ddc_execute(q, x, n, y, ld, ncols, mem, stream, true);
}
int ldsp_debug_ddc_tile(unsigned int D, unsigned int L, size_t* frames)
{
    return guard([&] {
        NONNULL(frames);
        ddc_check_decim(D);
        LDSP_REQUIRE(L >= 1, "ddc: at least one tap");
        decim_check_taps("ddc", L, D, false);
        *frames = (size_t)k::ddc_frames((int)D, (int)L);
    });
}

// ---------------------------------------------------------------- FMBank
static ldsp_fmbank_s* fmbank_make(unsigned int C, float kf, unsigned int D, std::vector<float> h, float scale)
{
    std::unique_ptr<ldsp_fmbank_s> o(new ldsp_fmbank_s());
    o->C = C;
    o->D = D;
    o->ref = (float)(1.0 / (2 * M_PI * (double)kf));   // as ldsp_freqdem_create
    o->h = std::move(h);
    o->scale = scale;
    return o.release();
}
static void fmbank_check_shape(unsigned int C, float kf, unsigned int D)
{
    LDSP_REQUIRE(C >= 1 && C <= (unsigned)k::kFmbankMaxC,
                 "fmbank: the row count must lie in 1 .. " + std::to_string(k::kFmbankMaxC));
    LDSP_REQUIRE(kf > 0.0f, "fmbank: kf must be > 0");
    LDSP_REQUIRE(D >= 1 && D <= (unsigned)k::kFmbankMaxD,
                 "fmbank: the decimation must lie in 1 .. " + std::to_string(k::kFmbankMaxD));
}
int ldsp_fmbank_create(unsigned int C, float kf, unsigned int D, unsigned int m, float fc, float as, ldsp_fmbank_t* q)
{
    return guard([&] {
        NONNULL(q);
        fmbank_check_shape(C, kf, D);
        auto p = decim_prototype("fmbank", D, m, fc, as);     // D = 1: the discriminator alone
        *q = fmbank_make(C, kf, D, std::move(p.first), p.second);
    });
}
int ldsp_fmbank_create_taps(unsigned int C, float kf, unsigned int D, const float* h, unsigned int L, ldsp_fmbank_t* q)
{
    return guard([&] {
        NONNULL(q);
        fmbank_check_shape(C, kf, D);
        LDSP_REQUIRE(L >= 1, "fmbank: at least one tap");
        NONNULL(h);
        decim_check_taps("fmbank", L, D, true);
        *q = fmbank_make(C, kf, D, std::vector<float>(h, h + L), 1.0f);
    });
}
int ldsp_fmbank_destroy(ldsp_fmbank_t q) { return guard([&] { destroy(q); }); }
int ldsp_fmbank_reset(ldsp_fmbank_t q)
{
    return guard([&] {
        NONNULL(q);
        q->seen = 0;
        q->at_rest([&] { q->zero_state(q->device); });
    });
}
int ldsp_fmbank_get_info(ldsp_fmbank_t q, unsigned int* C, unsigned int* D, unsigned int* L, unsigned int* skip)
{
    return guard([&] {
        NONNULL(q);
        if (C) *C = q->C;
        if (D) *D = q->D;
        if (L) *L = (unsigned)q->h.size();
        if (skip) *skip = (unsigned)q->skip();
    });
}
int ldsp_fmbank_get_taps(ldsp_fmbank_t q, float* h)
{
    return guard([&] {
        NONNULL(q);
        NONNULL(h);
        std::copy(q->h.begin(), q->h.end(), h);
    });
}
int ldsp_fmbank_get_scale(ldsp_fmbank_t q, float* s) { return guard([&] { NONNULL(q); NONNULL(s); *s = q->scale; }); }
int ldsp_fmbank_set_scale(ldsp_fmbank_t q, float s)
{
    return guard([&] {
        NONNULL(q);
        LDSP_REQUIRE(!q->h.empty(), "fmbank: the discriminator alone has no scale");
        q->scale = s;
    });
}
int ldsp_fmbank_num_outputs(ldsp_fmbank_t q, size_t K, size_t* ncols)
{
    return guard([&] {
        NONNULL(q);
        NONNULL(ncols);
        *ncols = q->num_outputs(K);
    });
}
int ldsp_fmbank_execute(ldsp_fmbank_t q, const void* x, size_t ldx, size_t K, void* y, size_t ldy, size_t* ncols, int mem,
                        void* stream)
{
    LDSP_RANGE("ldsp_fmbank_execute");
    return guard([&] {
        NONNULL(q);
        const size_t N = q->num_outputs(K);
        if (ncols) *ncols = N;
        LDSP_REQUIRE(ldx >= K, "fmbank_execute: input row stride below the number of samples");
        if (N > ldy) throw Error(LDSP_ERANGE, "fmbank_execute: output row stride below the number of output columns");
        LDSP_REQUIRE(K == 0 || x, "fmbank_execute: NULL input");
        LDSP_REQUIRE(N == 0 || y, "fmbank_execute: NULL output");
        Call call(*q, mem, x, stream);
        const Exec& e = call.e;
        const size_t C = q->C;
        // a host-memory call reads and writes dense [C][K] and [C][N] device images
        // (rows of the caller's images are ldx and ldy samples apart)
        const void* dx = q->stg.dev_in(e, x, K * 8, C, ldx * 8);
        float* dy = (float*)q->stg.dev_out(e, y, C * N * 4);
        if (K > 0) {
            k::FmbankCall c;
            c.x = dx;
            c.dhist = (const float*)q->dhist.in();
            c.dhist_out = (float*)q->dhist.out();
            c.prev = q->prev.in();
            c.prev_out = q->prev.out();
            c.n = K;
            c.ldx = e.host ? K : ldx;
            c.skip = q->skip();
            c.ncols = N;
            c.ldy = e.host ? N : ldy;
            c.C = (int)C;
            c.L = (int)q->h.size();
            c.taps = q->dtaps.as<float>();
            c.ref = q->ref;
            c.scale = q->scale;
            c.y = dy;
            k::fmbank((int)q->D, c, e.stream);
            q->dhist.flip();
            q->prev.flip();
            q->seen += K;
        }
        call.end();
        q->stg.finish(e, y, N * 4, C, ldy * 4);
    });
}
int ldsp_debug_fmbank_tile(unsigned int D, unsigned int L, size_t* frames)
{
    return guard([&] {
        NONNULL(frames);
        LDSP_REQUIRE(D >= 1 && D <= (unsigned)k::kFmbankMaxD,
                     "fmbank: the decimation must lie in 1 .. " + std::to_string(k::kFmbankMaxD));
        decim_check_taps("fmbank", L, D, false);
        *frames = L == 0 ? 256 : (size_t)k::fmbank_frames((int)D, (int)L);
    });
}

// ---------------------------------------------------------------- AudioBank
int ldsp_audiobank_create(unsigned int C, float rate, unsigned int m, float fc, float as, unsigned int npfb,
                          float sample_rate, double tau, int pcm16, ldsp_audiobank_t* q)
{
    return guard([&] {
        NONNULL(q);
        const bool de = sample_rate > 0.0f;
        LDSP_REQUIRE(C >= 1 && C <= (unsigned)k::kAudiobankMaxC,
                     "audiobank: the row count must lie in 1 .. " + std::to_string(k::kAudiobankMaxC));
        LDSP_REQUIRE(rate > 0.0f, "audiobank: resampling rate must be greater than zero");
        LDSP_REQUIRE(m > 0, "audiobank: filter semi-length must be greater than zero");
        LDSP_REQUIRE(fc > 0.0f && fc < 0.5f, "audiobank: filter cutoff must be in (0, 0.5)");
        LDSP_REQUIRE(as > 0.0f, "audiobank: filter stop-band suppression must be greater than zero");
        LDSP_REQUIRE(npfb > 0, "audiobank: number of filters must be greater than zero");
        LDSP_REQUIRE(!de || tau > 0.0, "audiobank: the de-emphasis time constant must be greater than zero");
        if (!(rate >= 1.0f / 32 && rate <= 4.0f))
            throw Error(LDSP_EUNSUP, "audiobank: a rate outside [1/32, 4] is not implemented");
        if (m > (unsigned)k::kAudiobankMaxM)
            throw Error(LDSP_EUNSUP, "audiobank: semi-length above " + std::to_string(k::kAudiobankMaxM) +
                                         " is not implemented");
        uint64_t np2 = 1;
        while (np2 < npfb) np2 <<= 1;                  // liquid_nextpow2
        if (np2 * 2 * m > (uint64_t)k::kAudiobankMaxTaps)
            throw Error(LDSP_EUNSUP, "audiobank: more than " + std::to_string(k::kAudiobankMaxTaps) +
                                         " branch taps (nfilter * 2 len) is not implemented");
        if (de && tau * (double)sample_rate > 32.0)
            throw Error(LDSP_EUNSUP, "audiobank: a time constant above 32 input samples is not implemented");
        std::unique_ptr<ldsp_audiobank_s> o(new ldsp_audiobank_s());
        o->C = C;
        o->m = m;
        o->rate = rate;
        o->step = (uint32_t)round((double)((float)(1 << 24) / rate));   // ResampObj::set_rate
        ResampDesign d = resamp_design(m, fc, as, npfb, 1);
        o->npfb = d.npfb;
        o->bits_index = d.bits_index;
        o->sub_len = d.sub_len;
        o->hproto = std::move(d.hproto);
        o->sub = std::move(d.sub);
        o->pcm16 = pcm16 != 0;
        if (de) {
            // DeemphasisFilter's coefficients (reference src/iirfilter.hpp:366-372) at any tau
            o->sample_rate = sample_rate;
            o->tau = tau;
            o->a = (float)exp(-1.0 / (tau * (double)sample_rate));
            o->b0 = (float)(1.0 - (double)o->a);
            // the warm-up: the smallest J with a^J <= 2^-30
            int J = 1;
            if (o->a > 0.0f) {
                J = std::max(1, (int)ceil(30.0 * M_LN2 / -log((double)o->a)));
                while (pow((double)o->a, J) > ldexp(1.0, -30)) J++;
            }
            o->J = k::audiobank_warmup(J);
            LDSP_REQUIRE(o->J <= k::kAudiobankMaxJ, "audiobank: de-emphasis warm-up out of range");
        }
        o->H = k::audiobank_hist((int)o->sub_len, o->J);
        *q = o.release();
    });
}
int ldsp_audiobank_destroy(ldsp_audiobank_t q) { return guard([&] { destroy(q); }); }
int ldsp_audiobank_reset(ldsp_audiobank_t q)
{
    return guard([&] {
        NONNULL(q);
        q->phase = 0;
        q->seen = 0;
        q->at_rest([&] { q->hist.zero(q->hist_bytes(), q->device); });
    });
}
int ldsp_audiobank_get_info(ldsp_audiobank_t q, unsigned int* C, unsigned int* npfb, uint32_t* step, uint32_t* phase,
                            unsigned int* sub_len)
{
    return guard([&] {
        NONNULL(q);
        if (C) *C = q->C;
        if (npfb) *npfb = q->npfb;
        if (step) *step = q->step;
        if (phase) *phase = (uint32_t)q->phase;
        if (sub_len) *sub_len = q->sub_len;
    });
}
int ldsp_audiobank_get_taps(ldsp_audiobank_t q, float* h, unsigned int cap, unsigned int* n)
{
    return guard([&] {
        NONNULL(q);
        if (n) *n = (unsigned)q->hproto.size();
        if (h) {
            LDSP_REQUIRE(cap >= q->hproto.size(), "audiobank_get_taps: capacity too small");
            std::copy(q->hproto.begin(), q->hproto.end(), h);
        }
    });
}
int ldsp_audiobank_get_coefs(ldsp_audiobank_t q, float* b0, float* a, float* sample_rate, double* tau)
{
    return guard([&] {
        NONNULL(q);
        if (b0) *b0 = q->b0;
        if (a) *a = q->a;
        if (sample_rate) *sample_rate = q->sample_rate;
        if (tau) *tau = q->tau;
    });
}
int ldsp_audiobank_get_scale(ldsp_audiobank_t q, float* s) { return guard([&] { NONNULL(q); NONNULL(s); *s = q->scale; }); }
int ldsp_audiobank_set_scale(ldsp_audiobank_t q, float s) { return guard([&] { NONNULL(q); q->scale = s; }); }
int ldsp_audiobank_num_outputs(ldsp_audiobank_t q, size_t K, size_t* nout)
{
    return guard([&] { NONNULL(q); NONNULL(nout); *nout = q->num_outputs(K); });
}
int ldsp_audiobank_execute(ldsp_audiobank_t q, const void* x, size_t ldx, size_t K, void* y, size_t ldy, size_t* nout,
                           int mem, void* stream)
{
    LDSP_RANGE("ldsp_audiobank_execute");
    return guard([&] {
        NONNULL(q);
        const size_t N = q->num_outputs(K);
        if (nout) *nout = N;
        LDSP_REQUIRE(ldx >= K, "audiobank_execute: input row stride below the number of samples");
        if (N > ldy) throw Error(LDSP_ERANGE, "audiobank_execute: output row stride below the number of outputs");
        LDSP_REQUIRE(K == 0 || x, "audiobank_execute: NULL input");
        LDSP_REQUIRE(N == 0 || y, "audiobank_execute: NULL output");
        Call call(*q, mem, x, stream);
        const Exec& e = call.e;
        const size_t C = q->C, osz = q->osz();
        // a host-memory call reads and writes dense [C][K] and [C][N] device images
        const void* dx = q->stg.dev_in(e, x, K * 4, C, ldx * 4);
        void* dy = q->stg.dev_out(e, y, C * N * osz);
        if (K > 0) {
            k::AudiobankCall c;
            c.x = (const float*)dx;
            c.hist = (const float*)q->hist.in();
            c.hist_out = (float*)q->hist.out();
            c.n = K;
            c.ldx = e.host ? K : ldx;
            c.K = N;
            c.ldy = e.host ? N : ldy;
            c.P0 = q->phase;
            c.seen = q->seen;
            c.step = q->step;
            c.bits_index = q->bits_index;
            c.sub_len = (int)q->sub_len;
            c.npfb = (int)q->npfb;
            c.C = (int)C;
            c.J = q->J;
            c.H = q->H;
            c.a = (double)q->a;
            c.b0 = (double)q->b0;
            c.sub = q->dsub.as<float>();
            c.scale = q->scale;
            c.pcm16 = q->pcm16 ? 1 : 0;
            c.y = dy;
            k::audiobank(c, e.stream);
            q->hist.flip();
            q->phase = (uint64_t)((long long)q->phase + (long long)N * q->step - (long long)K * (1LL << 24));
            q->seen += K;
        }
        call.end();
        q->stg.finish(e, y, N * osz, C, ldy * osz);
    });
}
int ldsp_debug_audiobank_tile(ldsp_audiobank_t q, size_t* outputs)
{
    return guard([&] {
        NONNULL(q);
        NONNULL(outputs);
        *outputs = (size_t)q->tile();
    });
}

// ---------------------------------------------------------------- SquelchBank
// thr = (float) 10^(dB / 10), the power in double
static void sqbank_thresholds(const double* dB, unsigned int n, unsigned int C, std::vector<double>& db, std::vector<float>& lin)
{
    NONNULL(dB);
    LDSP_REQUIRE(n == 1 || n == C, "sqbank: one threshold or one per row");
    for (unsigned i = 0; i < n; i++) LDSP_REQUIRE(std::isfinite(dB[i]), "sqbank: thresholds must be finite");
    db.resize(C);
    lin.resize(C);
    for (unsigned c = 0; c < C; c++) {
        db[c] = dB[n == 1 ? 0 : c];
        lin[c] = (float)pow(10.0, db[c] / 10.0);
    }
}
int ldsp_sqbank_create(unsigned int C, unsigned int B, double alpha, double threshold_dB, unsigned int timeout,
                       ldsp_sqbank_t* q)
{
    return guard([&] {
        NONNULL(q);
        LDSP_REQUIRE(C >= 1 && C <= (unsigned)k::kSqbankMaxC,
                     "sqbank: the row count must lie in 1 .. " + std::to_string(k::kSqbankMaxC));
        LDSP_REQUIRE(B >= (unsigned)k::kSqbankMinB && B <= (unsigned)k::kSqbankMaxB,
                     "sqbank: the block length must lie in " + std::to_string(k::kSqbankMinB) + " .. " +
                         std::to_string(k::kSqbankMaxB));
        LDSP_REQUIRE(alpha > 0.0 && alpha <= 1.0, "sqbank: the bandwidth must lie in (0, 1]");
        LDSP_REQUIRE(timeout >= 1 && timeout <= (unsigned)INT32_MAX, "sqbank: the timeout must be at least one block");
        std::unique_ptr<ldsp_sqbank_s> o(new ldsp_sqbank_s());
        o->C = C;
        o->B = B;
        o->alpha = alpha;
        o->timeout = timeout;
        sqbank_thresholds(&threshold_dB, 1, C, o->thr_db, o->thr);
        *q = o.release();
    });
}
int ldsp_sqbank_destroy(ldsp_sqbank_t q) { return guard([&] { destroy(q); }); }
int ldsp_sqbank_reset(ldsp_sqbank_t q)
{
    return guard([&] {
        NONNULL(q);
        q->seen = 0;
        q->at_rest([&] { q->zero_state(q->device); });
    });
}
int ldsp_sqbank_set_thresholds(ldsp_sqbank_t q, const double* dB, unsigned int n)
{
    return guard([&] {
        NONNULL(q);
        std::vector<double> db;
        std::vector<float> lin;
        sqbank_thresholds(dB, n, q->C, db, lin);
        // the table changes only once the object's earlier calls have finished with it
        q->at_rest([&] { ldsp::upload(q->dthr, lin, q->device); });
        q->thr_db = std::move(db);
        q->thr = std::move(lin);
    });
}
int ldsp_sqbank_get_thresholds(ldsp_sqbank_t q, double* dB, float* lin)
{
    return guard([&] {
        NONNULL(q);
        if (dB) std::copy(q->thr_db.begin(), q->thr_db.end(), dB);
        if (lin) std::copy(q->thr.begin(), q->thr.end(), lin);
    });
}
int ldsp_sqbank_get_info(ldsp_sqbank_t q, unsigned int* C, unsigned int* B, double* alpha, unsigned int* timeout,
                         unsigned int* fill)
{
    return guard([&] {
        NONNULL(q);
        if (C) *C = q->C;
        if (B) *B = q->B;
        if (alpha) *alpha = q->alpha;
        if (timeout) *timeout = q->timeout;
        if (fill) *fill = (unsigned)q->fill();
    });
}
int ldsp_sqbank_num_outputs(ldsp_sqbank_t q, size_t K, size_t* nblocks)
{
    return guard([&] {
        NONNULL(q);
        NONNULL(nblocks);
        *nblocks = q->num_outputs(K);
    });
}
int ldsp_sqbank_execute(ldsp_sqbank_t q, const void* x, size_t ldx, size_t K, uint8_t* status, size_t lds, float* level,
                        size_t ldl, void* y, size_t ldy, size_t* nblocks, int mem, void* stream)
{
    LDSP_RANGE("ldsp_sqbank_execute");
    return guard([&] {
        NONNULL(q);
        const size_t N = q->num_outputs(K), B = q->B;
        if (nblocks) *nblocks = N;
        LDSP_REQUIRE(ldx >= K, "sqbank_execute: input row stride below the number of samples");
        if (N > lds || N > ldl) throw Error(LDSP_ERANGE, "sqbank_execute: status or level row stride below the number of blocks");
        if (y && N * B > ldy) throw Error(LDSP_ERANGE, "sqbank_execute: output row stride below the blocks' samples");
        LDSP_REQUIRE(K == 0 || x, "sqbank_execute: NULL input");
        LDSP_REQUIRE(N == 0 || (status && level), "sqbank_execute: NULL status or level");
        Call call(*q, mem, x, stream);
        const Exec& e = call.e;
        const size_t C = q->C;
        // a host-memory call reads and writes dense device images (rows of the caller's
        // images are ldx, lds, ldl and ldy elements apart)
        const void* dx = q->stg.dev_in(e, x, K * 8, C, ldx * 8);
        uint8_t* dstat = (uint8_t*)q->stg_status.dev_out(e, status, C * N);
        float* dlev = (float*)q->stg_level.dev_out(e, level, C * N * 4);
        void* dy = y ? q->stg.dev_out(e, y, C * N * B * 8) : nullptr;
        if (K > 0) {
            k::SqbankCall c;
            c.x = dx;
            c.hist = q->hist.in();
            c.hist_out = q->hist.out();
            c.n = K;
            c.ldx = e.host ? K : ldx;
            c.fill = q->fill();
            c.nblocks = N;
            c.lds = e.host ? N : lds;
            c.ldl = e.host ? N : ldl;
            c.ldy = e.host ? N * B : ldy;
            c.C = (int)C;
            c.B = (int)B;
            c.timeout = (int)q->timeout;
            c.alpha = q->alpha;
            c.thr = q->dthr.as<float>();
            c.st = q->dstate.as<k::SqState>();
            c.p = (double*)q->dpow.ensure(std::max<size_t>(C * N, 1) * 8, e.device);
            c.status = dstat;
            c.level = dlev;
            c.y = dy;
            k::sqbank(c, e.stream);
            q->hist.flip();
            q->seen += K;
        }
        call.end();
        q->stg_status.finish(e, status, N, C, lds);
        q->stg_level.finish(e, level, N * 4, C, ldl * 4);
        if (y) q->stg.finish(e, y, N * B * 8, C, ldy * 8);
    });
}
int ldsp_sqbank_get_state(ldsp_sqbank_t q, int* mode, unsigned int* timer, double* s)
{
    return guard([&] {
        NONNULL(q);
        std::vector<k::SqState> st(q->C, ldsp_sqbank_s::initial());
        q->at_rest([&] { LDSP_HIP(hipMemcpy(st.data(), q->dstate.p, st.size() * sizeof(k::SqState), hipMemcpyDeviceToHost)); });
        for (unsigned c = 0; c < q->C; c++) {
            if (mode) mode[c] = st[c].mode;
            if (timer) timer[c] = (unsigned)st[c].timer;
            if (s) s[c] = st[c].s;
        }
    });
}
int ldsp_debug_sqbank_tile(unsigned int B, size_t* blocks)
{
    return guard([&] {
        NONNULL(blocks);
        LDSP_REQUIRE(B >= (unsigned)k::kSqbankMinB && B <= (unsigned)k::kSqbankMaxB,
                     "sqbank: the block length must lie in " + std::to_string(k::kSqbankMinB) + " .. " +
                         std::to_string(k::kSqbankMaxB));
        *blocks = (size_t)k::sqbank_tile((int)B);
    });
}

// ---------------------------------------------------------------- AGCBank
// dB -> units of 2^-24 octave of amplitude: llrint(v 2^24 / (20 log10 2)) in double
static int64_t agcbank_units(double dB) { return (int64_t)llrint(dB * agc::kAgcQ / (20.0 * log10(2.0))); }
static const double kAgcbankMaxDb = 180.0;            // |target| and |max_gain|: within +-30 octaves
int ldsp_agcbank_create(unsigned int C, unsigned int B, const double* target_dB, unsigned int ntarget, double max_gain_dB,
                        unsigned int hang, double decay_dB, int cplx, ldsp_agcbank_t* q)
{
    return guard([&] {
        NONNULL(q);
        LDSP_REQUIRE(C >= 1 && C <= (unsigned)k::kAgcbankMaxC,
                     "agcbank: the row count must lie in 1 .. " + std::to_string(k::kAgcbankMaxC));
        LDSP_REQUIRE(B >= (unsigned)k::kAgcbankMinB && B <= (unsigned)k::kAgcbankMaxB,
                     "agcbank: the block length must lie in " + std::to_string(k::kAgcbankMinB) + " .. " +
                         std::to_string(k::kAgcbankMaxB));
        LDSP_REQUIRE(hang <= (unsigned)agc::kAgcMaxHang,
                     "agcbank: the hang must lie in 0 .. " + std::to_string(agc::kAgcMaxHang) + " blocks");
        LDSP_REQUIRE(std::isfinite(decay_dB) && decay_dB >= 0.0, "agcbank: the decay must be at or above 0 dB per block");
        LDSP_REQUIRE(std::isfinite(max_gain_dB) && std::fabs(max_gain_dB) <= kAgcbankMaxDb,
                     "agcbank: max_gain must lie within +-180 dB");
        LDSP_REQUIRE(cplx == 0 || cplx == 1, "agcbank: cplx must be 0 or 1");
        NONNULL(target_dB);
        LDSP_REQUIRE(ntarget == 1 || ntarget == C, "agcbank: one target or one per row");
        for (unsigned i = 0; i < ntarget; i++)
            LDSP_REQUIRE(std::isfinite(target_dB[i]) && std::fabs(target_dB[i]) <= kAgcbankMaxDb,
                         "agcbank: targets must lie within +-180 dB");
        std::unique_ptr<ldsp_agcbank_s> o(new ldsp_agcbank_s());
        o->C = C;
        o->B = B;
        o->H = hang;
        o->cplx = cplx != 0;
        o->max_gain_db = max_gain_dB;
        o->decay_db = decay_dB;
        o->Gmax = (int32_t)agcbank_units(max_gain_dB);
        // a decay of the whole range per block or more acts as the whole range
        o->d = decay_dB >= 800.0 ? (int64_t)1 << 31 : std::min<int64_t>(agcbank_units(decay_dB), (int64_t)1 << 31);
        o->target_db.resize(C);
        o->T.resize(C);
        for (unsigned c = 0; c < C; c++) {
            o->target_db[c] = target_dB[ntarget == 1 ? 0 : c];
            o->T[c] = (int32_t)agcbank_units(o->target_db[c]);
        }
        *q = o.release();
    });
}
int ldsp_agcbank_destroy(ldsp_agcbank_t q) { return guard([&] { destroy(q); }); }
int ldsp_agcbank_reset(ldsp_agcbank_t q)
{
    return guard([&] {
        NONNULL(q);
        q->seen = 0;
        q->at_rest([&] { q->zero_state(q->device); });
    });
}
int ldsp_agcbank_get_info(ldsp_agcbank_t q, unsigned int* C, unsigned int* B, unsigned int* hang, double* decay_dB,
                          double* max_gain_dB, double* target_dB, int* cplx, unsigned int* fill)
{
    return guard([&] {
        NONNULL(q);
        if (C) *C = q->C;
        if (B) *B = q->B;
        if (hang) *hang = q->H;
        if (decay_dB) *decay_dB = q->decay_db;
        if (max_gain_dB) *max_gain_dB = q->max_gain_db;
        if (target_dB) std::copy(q->target_db.begin(), q->target_db.end(), target_dB);
        if (cplx) *cplx = q->cplx ? 1 : 0;
        if (fill) *fill = (unsigned)q->fill();
    });
}
int ldsp_agcbank_num_outputs(ldsp_agcbank_t q, size_t K, size_t* tracked, size_t* emitted)
{
    return guard([&] {
        NONNULL(q);
        LDSP_REQUIRE(tracked || emitted, "agcbank_num_outputs: tracked and emitted are both NULL");
        if (tracked) *tracked = (size_t)(q->tracked(q->seen + K) - q->tracked(q->seen));
        if (emitted) *emitted = (size_t)(q->emitted(q->seen + K) - q->emitted(q->seen));
    });
}
int ldsp_agcbank_execute(ldsp_agcbank_t q, const void* x, size_t ldx, size_t K, void* y, size_t ldy, int32_t* peak_q,
                         int32_t* gain_q, size_t ldq, size_t* nw, int mem, void* stream)
{
    LDSP_RANGE("ldsp_agcbank_execute");
    return guard([&] {
        NONNULL(q);
        const size_t B = q->B, esz = q->esz();
        const size_t nt = (size_t)(q->tracked(q->seen + K) - q->tracked(q->seen));
        const size_t ne = (size_t)(q->emitted(q->seen + K) - q->emitted(q->seen));
        if (nw) *nw = ne * B;
        LDSP_REQUIRE(ldx >= K, "agcbank_execute: input row stride below the number of samples");
        if (ne * B > ldy) throw Error(LDSP_ERANGE, "agcbank_execute: output row stride below the emitted samples");
        if (nt > ldq) throw Error(LDSP_ERANGE, "agcbank_execute: peak_q / gain_q row stride below the tracked blocks");
        LDSP_REQUIRE(K == 0 || x, "agcbank_execute: NULL input");
        LDSP_REQUIRE(ne == 0 || y, "agcbank_execute: NULL output");
        LDSP_REQUIRE(nt == 0 || (peak_q && gain_q), "agcbank_execute: NULL peak_q or gain_q");
        Call call(*q, mem, x, stream);
        const Exec& e = call.e;
        const size_t C = q->C;
        // a host-memory call reads and writes dense device images (rows of the caller's
        // images are ldx, ldy and ldq elements apart)
        const void* dx = q->stg.dev_in(e, x, K * esz, C, ldx * esz);
        void* dy = q->stg.dev_out(e, y, C * ne * B * esz);
        int32_t* dpq = (int32_t*)q->stg_peak.dev_out(e, peak_q, C * nt * 4);
        int32_t* dgq = (int32_t*)q->stg_gain.dev_out(e, gain_q, C * nt * 4);
        if (K > 0) {
            k::AgcbankCall c;
            c.x = dx;
            c.hist = q->hist.in();
            c.hist_out = q->hist.out();
            c.n = K;
            c.ldx = e.host ? K : ldx;
            c.fill = q->fill();
            c.pend = q->pend();
            c.nt = nt;
            c.ne = ne;
            c.ldq = e.host ? nt : ldq;
            c.ldg = nt + 2;
            c.ldy = e.host ? ne * B : ldy;
            c.C = (int)C;
            c.B = (int)B;
            c.H = (int)q->H;
            c.cplx = q->cplx ? 1 : 0;
            c.Gmax = q->Gmax;
            c.d = q->d;
            c.target = q->dtarget.as<int32_t>();
            c.level = q->dlevel.as<int32_t>();
            c.tail = q->dtail.as<int32_t>();
            c.edge = q->dedge.as<float>();
            c.peak_q = dpq;
            c.gain_q = dgq;
            c.gains = (float*)q->dgains.ensure(C * (nt + 2) * 4, e.device);
            c.y = dy;
            k::agcbank(c, e.stream);
            q->hist.flip();
            q->seen += K;
        }
        call.end();
        q->stg.finish(e, y, ne * B * esz, C, ldy * esz);
        q->stg_peak.finish(e, peak_q, nt * 4, C, ldq * 4);
        q->stg_gain.finish(e, gain_q, nt * 4, C, ldq * 4);
    });
}
int ldsp_agcbank_get_state(ldsp_agcbank_t q, int32_t* level, int32_t* peaks, float* gains)
{
    return guard([&] {
        NONNULL(q);
        const size_t C = q->C, H = q->H, TL = (size_t)k::kAgcbankTail;
        std::vector<int32_t> lv(C, agc::kAgcFloor), tl(C * TL, agc::kAgcFloor);
        std::vector<float> ed(C * 2, 0.0f);
        q->at_rest([&] {
            LDSP_HIP(hipMemcpy(lv.data(), q->dlevel.p, lv.size() * 4, hipMemcpyDeviceToHost));
            LDSP_HIP(hipMemcpy(tl.data(), q->dtail.p, tl.size() * 4, hipMemcpyDeviceToHost));
            LDSP_HIP(hipMemcpy(ed.data(), q->dedge.p, ed.size() * 4, hipMemcpyDeviceToHost));
        });
        if (level) std::copy(lv.begin(), lv.end(), level);
        if (peaks)
            for (size_t c = 0; c < C; c++) std::copy_n(&tl[c * TL + TL - H], H, peaks + c * H);
        if (gains) std::copy(ed.begin(), ed.end(), gains);
    });
}
int ldsp_debug_agcbank_units(double dB, int64_t* units)
{
    return guard([&] {
        NONNULL(units);
        LDSP_REQUIRE(std::isfinite(dB) && std::fabs(dB) <= 1.0e9, "agcbank: dB out of range");
        *units = agcbank_units(dB);
    });
}
int ldsp_debug_agcbank_track(const int32_t* peak_q, size_t n, unsigned int hang, int64_t d, size_t width, int32_t* level,
                             int32_t* peaks, int32_t* L)
{
    return guard([&] {
        NONNULL(level);
        LDSP_REQUIRE(n == 0 || (peak_q && L), "agcbank_track: NULL peak_q or L");
        LDSP_REQUIRE(hang <= (unsigned)agc::kAgcMaxHang, "agcbank_track: the hang must lie in 0 .. 255 blocks");
        LDSP_REQUIRE(hang == 0 || peaks, "agcbank_track: NULL peaks");
        LDSP_REQUIRE(d >= 0 && d <= ((int64_t)1 << 31), "agcbank_track: the decay must lie in 0 .. 2^31 units");
        LDSP_REQUIRE(width >= 1, "agcbank_track: the partition width must be at least 1");
        LDSP_REQUIRE(n <= ((size_t)1 << 31), "agcbank_track: too many blocks");
        auto in_range = [](int32_t v) { return v >= agc::kAgcFloor && v <= agc::kAgcCeil; };
        LDSP_REQUIRE(in_range(*level), "agcbank_track: level out of range");
        for (unsigned i = 0; i < hang; i++) LDSP_REQUIRE(in_range(peaks[i]), "agcbank_track: peaks out of range");
        for (size_t i = 0; i < n; i++) LDSP_REQUIRE(in_range(peak_q[i]), "agcbank_track: peak_q out of range");
        if (n == 0) return;
        agc::agc_track_partitioned(peak_q, n, hang, d, width, level, peaks, L);
    });
}

// ---------------------------------------------------------------- ToneBank
static std::string tonebank_block_text()
{
    return "tonebank: the block length must be a multiple of 64 in " + std::to_string(k::kTonebankMinB) + " .. " +
           std::to_string(k::kTonebankMaxB);
}
static void tonebank_want(const int* want, unsigned int n, unsigned int C, unsigned int F, std::vector<int8_t>& out)
{
    NONNULL(want);
    LDSP_REQUIRE(n == 1 || n == C, "tonebank: one wanted tone or one per row");
    for (unsigned i = 0; i < n; i++)
        LDSP_REQUIRE(want[i] >= -1 && want[i] < (int)F, "tonebank: want must lie in -1 .. F - 1");
    out.resize(C);
    for (unsigned c = 0; c < C; c++) out[c] = (int8_t)want[n == 1 ? 0 : c];
}
int ldsp_tonebank_create(unsigned int C, const double* tones, unsigned int F, unsigned int B, int window, double dominance,
                         float floor, unsigned int hold, ldsp_tonebank_t* q)
{
    return guard([&] {
        NONNULL(q);
        LDSP_REQUIRE(C >= 1 && C <= (unsigned)k::kTonebankMaxC,
                     "tonebank: the row count must lie in 1 .. " + std::to_string(k::kTonebankMaxC));
        LDSP_REQUIRE(F >= (unsigned)k::kTonebankMinF && F <= (unsigned)k::kTonebankMaxF,
                     "tonebank: the number of tones must lie in " + std::to_string(k::kTonebankMinF) + " .. " +
                         std::to_string(k::kTonebankMaxF));
        NONNULL(tones);
        for (unsigned i = 0; i < F; i++)
            LDSP_REQUIRE(std::isfinite(tones[i]) && tones[i] > 0.0 && tones[i] < 0.5,
                         "tonebank: tones must lie in (0, 0.5) cycles per sample");
        LDSP_REQUIRE(B >= (unsigned)k::kTonebankMinB && B <= (unsigned)k::kTonebankMaxB && B % 64 == 0,
                     tonebank_block_text());
        LDSP_REQUIRE(window == LDSP_TONE_RECT || window == LDSP_TONE_HANN, "tonebank: unknown window");
        LDSP_REQUIRE(dominance >= 1.0 && std::isfinite(dominance), "tonebank: the dominance must be finite and >= 1");
        LDSP_REQUIRE(floor >= 0.0f && std::isfinite(floor), "tonebank: the floor must be finite and >= 0");
        LDSP_REQUIRE(hold <= (unsigned)k::kTonebankMaxHold,
                     "tonebank: the hold must lie in 0 .. " + std::to_string(k::kTonebankMaxHold) + " blocks");
        std::unique_ptr<ldsp_tonebank_s> o(new ldsp_tonebank_s());
        o->C = C;
        o->F = F;
        o->B = B;
        o->window = window;
        o->dominance = dominance;
        o->floor = floor;
        o->hold = hold;
        o->tones.assign(tones, tones + F);
        o->want.assign(C, (int8_t)-1);
        // the tables in double, each entry rounded once
        const double two_pi = 2.0 * M_PI;
        std::vector<double> w(B, 1.0);
        if (window == LDSP_TONE_HANN)
            for (unsigned i = 0; i < B; i++) w[i] = 0.5 - 0.5 * cos(two_pi * (double)i / (double)B);
        double sum = 0.0;
        for (unsigned i = 0; i < B; i++) sum += w[i];
        o->sumw = sum;
        const double s = sqrt(2.0) / sum;
        o->tc.resize((size_t)F * B);
        o->ts.resize((size_t)F * B);
        for (unsigned kk = 0; kk < F; kk++)
            for (unsigned i = 0; i < B; i++) {
                const double ph = two_pi * tones[kk] * (double)i;
                o->tc[(size_t)kk * B + i] = (float)(s * w[i] * cos(ph));
                o->ts[(size_t)kk * B + i] = (float)(-s * w[i] * sin(ph));
            }
        *q = o.release();
    });
}
int ldsp_tonebank_destroy(ldsp_tonebank_t q) { return guard([&] { destroy(q); }); }
int ldsp_tonebank_reset(ldsp_tonebank_t q)
{
    return guard([&] {
        NONNULL(q);
        q->seen = 0;
        q->at_rest([&] { q->zero_state(q->device); });
    });
}
int ldsp_tonebank_get_info(ldsp_tonebank_t q, unsigned int* C, unsigned int* F, unsigned int* B, int* window,
                           unsigned int* hold, unsigned int* fill)
{
    return guard([&] {
        NONNULL(q);
        if (C) *C = q->C;
        if (F) *F = q->F;
        if (B) *B = q->B;
        if (window) *window = q->window;
        if (hold) *hold = q->hold;
        if (fill) *fill = (unsigned)q->fill();
    });
}
int ldsp_tonebank_get_tables(ldsp_tonebank_t q, double* tones, float* tc, float* ts, double* sumw)
{
    return guard([&] {
        NONNULL(q);
        if (tones) std::copy(q->tones.begin(), q->tones.end(), tones);
        if (tc) std::copy(q->tc.begin(), q->tc.end(), tc);
        if (ts) std::copy(q->ts.begin(), q->ts.end(), ts);
        if (sumw) *sumw = q->sumw;
    });
}
int ldsp_tonebank_set_want(ldsp_tonebank_t q, const int* want, unsigned int n)
{
    return guard([&] {
        NONNULL(q);
        std::vector<int8_t> w;
        tonebank_want(want, n, q->C, q->F, w);
        // the table changes only once the object's earlier calls have finished with it
        q->at_rest([&] { ldsp::upload(q->dwant, w, q->device); });
        q->want = std::move(w);
    });
}
int ldsp_tonebank_get_want(ldsp_tonebank_t q, int* want)
{
    return guard([&] {
        NONNULL(q);
        NONNULL(want);
        std::copy(q->want.begin(), q->want.end(), want);
    });
}
int ldsp_tonebank_set_dominance(ldsp_tonebank_t q, double dominance)
{
    return guard([&] {
        NONNULL(q);
        LDSP_REQUIRE(dominance >= 1.0 && std::isfinite(dominance), "tonebank: the dominance must be finite and >= 1");
        q->dominance = dominance;
    });
}
int ldsp_tonebank_get_dominance(ldsp_tonebank_t q, double* dominance)
{
    return guard([&] {
        NONNULL(q);
        NONNULL(dominance);
        *dominance = q->dominance;
    });
}
int ldsp_tonebank_set_floor(ldsp_tonebank_t q, float floor)
{
    return guard([&] {
        NONNULL(q);
        LDSP_REQUIRE(floor >= 0.0f && std::isfinite(floor), "tonebank: the floor must be finite and >= 0");
        q->floor = floor;
    });
}
int ldsp_tonebank_get_floor(ldsp_tonebank_t q, float* floor)
{
    return guard([&] {
        NONNULL(q);
        NONNULL(floor);
        *floor = q->floor;
    });
}
int ldsp_tonebank_num_outputs(ldsp_tonebank_t q, size_t K, size_t* nblocks)
{
    return guard([&] {
        NONNULL(q);
        NONNULL(nblocks);
        *nblocks = q->num_outputs(K);
    });
}
int ldsp_tonebank_execute(ldsp_tonebank_t q, const float* x, size_t ldx, size_t K, float* power, size_t ldp, int8_t* tone,
                          size_t ldt, uint8_t* open, size_t ldo, float* y, size_t ldy, size_t* nblocks, int mem,
                          void* stream)
{
    LDSP_RANGE("ldsp_tonebank_execute");
    return guard([&] {
        NONNULL(q);
        const size_t N = q->num_outputs(K), B = q->B, F = q->F;
        if (nblocks) *nblocks = N;
        LDSP_REQUIRE(ldx >= K, "tonebank_execute: input row stride below the number of samples");
        if (N * F > ldp) throw Error(LDSP_ERANGE, "tonebank_execute: power row stride below the blocks' tones");
        if (N > ldt || (open && N > ldo))
            throw Error(LDSP_ERANGE, "tonebank_execute: tone or open row stride below the number of blocks");
        if (y && N * B > ldy) throw Error(LDSP_ERANGE, "tonebank_execute: output row stride below the blocks' samples");
        LDSP_REQUIRE(K == 0 || x, "tonebank_execute: NULL input");
        LDSP_REQUIRE(N == 0 || (power && tone), "tonebank_execute: NULL power or tone");
        Call call(*q, mem, x, stream);
        const Exec& e = call.e;
        const size_t C = q->C;
        // a host-memory call reads and writes dense device images (rows of the caller's
        // images are ldx, ldp, ldt, ldo and ldy elements apart)
        const void* dx = q->stg.dev_in(e, x, K * 4, C, ldx * 4);
        float* dpow = (float*)q->stg_power.dev_out(e, power, C * N * F * 4);
        int8_t* dtone = (int8_t*)q->stg_tone.dev_out(e, tone, C * N);
        uint8_t* dopen = open ? (uint8_t*)q->stg_open.dev_out(e, open, C * N) : nullptr;
        void* dy = y ? q->stg.dev_out(e, y, C * N * B * 4) : nullptr;
        if (K > 0) {
            k::TonebankCall c;
            c.x = (const float*)dx;
            c.hist = (const float*)q->hist.in();
            c.hist_out = (float*)q->hist.out();
            c.tab = q->dtab.as<float>();
            c.n = K;
            c.ldx = e.host ? K : ldx;
            c.fill = q->fill();
            c.nblocks = N;
            c.ldp = e.host ? N * F : ldp;
            c.ldt = e.host ? N : ldt;
            c.ldo = e.host || !open ? N : ldo;
            c.ldy = e.host ? N * B : ldy;
            c.C = (int)C;
            c.B = (int)B;
            c.F = (int)F;
            c.hold = (int)q->hold;
            c.floor = q->floor;
            c.dominance = q->dominance;
            c.want = q->dwant.as<int8_t>();
            c.since = (const int*)q->since.in();
            c.since_out = (int*)q->since.out();
            c.power = dpow;
            c.tone = dtone;
            // the gate reads the flags: a call that takes none keeps them in the object
            c.open = dopen ? dopen : (uint8_t*)q->dopen.ensure(std::max<size_t>(C * N, 1), e.device);
            c.y = (float*)dy;
            k::tonebank(c, e.stream);
            q->hist.flip();
            if (N > 0) q->since.flip();
            q->seen += K;
        }
        call.end();
        q->stg_power.finish(e, power, N * F * 4, C, ldp * 4);
        q->stg_tone.finish(e, tone, N, C, ldt);
        if (open) q->stg_open.finish(e, open, N, C, ldo);
        if (y) q->stg.finish(e, y, N * B * 4, C, ldy * 4);
    });
}
int ldsp_tonebank_get_state(ldsp_tonebank_t q, int* since)
{
    return guard([&] {
        NONNULL(q);
        NONNULL(since);
        std::vector<int> st(q->C, k::kTonebankSat);
        q->at_rest([&] { LDSP_HIP(hipMemcpy(st.data(), q->since.in(), st.size() * sizeof(int), hipMemcpyDeviceToHost)); });
        std::copy(st.begin(), st.end(), since);
    });
}
int ldsp_debug_tonebank_tile(unsigned int B, size_t* columns)
{
    return guard([&] {
        NONNULL(columns);
        LDSP_REQUIRE(B >= (unsigned)k::kTonebankMinB && B <= (unsigned)k::kTonebankMaxB && B % 64 == 0,
                     tonebank_block_text());
        *columns = (size_t)k::tonebank_tile((int)B);
    });
}

// ---------------------------------------------------------------- StereoBank
// w = rint(pilot 2^32): the product is exact (a power of two), rint rounds ties to even; 0 < pilot < 0.25 keeps it below 2^30
static uint32_t stbank_check_shape(unsigned int C, double pilot, unsigned int D, float thr)
{
    LDSP_REQUIRE(C >= 1 && C <= (unsigned)k::kStbankMaxC,
                 "stbank: the row count must lie in 1 .. " + std::to_string(k::kStbankMaxC));
    LDSP_REQUIRE(pilot > 0.0 && pilot < 0.25, "stbank: the pilot frequency must lie in (0, 0.25) cycles per sample");
    LDSP_REQUIRE(D >= 1 && D <= (unsigned)k::kStbankMaxD,
                 "stbank: the decimation must lie in 1 .. " + std::to_string(k::kStbankMaxD));
    LDSP_REQUIRE(thr >= 0.0f, "stbank: the pilot threshold must be >= 0");
    return (uint32_t)(uint64_t)std::nearbyint(pilot * 4294967296.0);
}
static void stbank_check_length(unsigned int L)
{
    LDSP_REQUIRE(L >= 1 && L <= (unsigned)k::kStbankMaxL,
                 "stbank: the prototype length must lie in 1 .. " + std::to_string(k::kStbankMaxL));
}
static ldsp_stbank_s* stbank_make(unsigned int C, uint32_t w, unsigned int D, float thr, std::vector<float> h,
                                  std::vector<float> g)
{
    std::unique_ptr<ldsp_stbank_s> o(new ldsp_stbank_s());
    o->C = C;
    o->D = D;
    o->w = w;
    o->thr = thr;
    o->h = std::move(h);
    o->g = std::move(g);
    return o.release();
}
// firdes_kaiser(L, fc, as, 0) with every tap divided in double by the double sum of the float32 design, rounded once
static std::vector<float> stbank_design(unsigned int L, double fc, float as)
{
    std::vector<float> h = design::firdes_kaiser(L, (float)fc, as, 0.0f);
    double sum = 0.0;
    for (float v : h) sum += (double)v;
    for (float& v : h) v = (float)((double)v / sum);
    return h;
}
int ldsp_stbank_create(unsigned int C, double pilot, unsigned int D, unsigned int L, float as, float threshold,
                       ldsp_stbank_t* q)
{
    return guard([&] {
        NONNULL(q);
        const uint32_t w = stbank_check_shape(C, pilot, D, threshold);
        LDSP_REQUIRE(as > 0.0f, "stbank: stop-band attenuation must be > 0");
        if (L == 0) {                                 // the default length
            const double half = std::ceil(8.5 / pilot);
            if (2.0 * half + 1.0 > (double)k::kStbankMaxL)
                throw Error(LDSP_EUNSUP, "stbank: a default prototype above " + std::to_string(k::kStbankMaxL) +
                                             " taps is not implemented (pilot too low)");
            L = 2 * (unsigned)half + 1;
        }
        stbank_check_length(L);
        *q = stbank_make(C, w, D, threshold, stbank_design(L, 17.0 / 19.0 * pilot, as),
                         stbank_design(L, 2.0 / 19.0 * pilot, as));
    });
}
int ldsp_stbank_create_taps(unsigned int C, double pilot, unsigned int D, const float* h, unsigned int L, const float* g,
                            unsigned int Lg, float threshold, ldsp_stbank_t* q)
{
    return guard([&] {
        NONNULL(q);
        const uint32_t w = stbank_check_shape(C, pilot, D, threshold);
        stbank_check_length(L);
        LDSP_REQUIRE(Lg == L, "stbank: the audio and the pilot prototype must have the same length");
        NONNULL(h);
        NONNULL(g);
        *q = stbank_make(C, w, D, threshold, std::vector<float>(h, h + L), std::vector<float>(g, g + L));
    });
}
int ldsp_stbank_destroy(ldsp_stbank_t q) { return guard([&] { destroy(q); }); }
int ldsp_stbank_reset(ldsp_stbank_t q)
{
    return guard([&] {
        NONNULL(q);
        q->seen = 0;
        q->at_rest([&] { q->zero_state(q->device); });
    });
}
int ldsp_stbank_get_info(ldsp_stbank_t q, unsigned int* C, unsigned int* D, unsigned int* L, unsigned int* skip,
                         uint32_t* w)
{
    return guard([&] {
        NONNULL(q);
        if (C) *C = q->C;
        if (D) *D = q->D;
        if (L) *L = (unsigned)q->h.size();
        if (skip) *skip = (unsigned)q->skip();
        if (w) *w = q->w;
    });
}
int ldsp_stbank_get_taps(ldsp_stbank_t q, float* h, float* g)
{
    return guard([&] {
        NONNULL(q);
        if (h) std::copy(q->h.begin(), q->h.end(), h);
        if (g) std::copy(q->g.begin(), q->g.end(), g);
    });
}
int ldsp_stbank_get_threshold(ldsp_stbank_t q, float* t) { return guard([&] { NONNULL(q); NONNULL(t); *t = q->thr; }); }
int ldsp_stbank_set_threshold(ldsp_stbank_t q, float t)
{
    return guard([&] {
        NONNULL(q);
        LDSP_REQUIRE(t >= 0.0f, "stbank: the pilot threshold must be >= 0");
        q->thr = t;                                   // a kernel argument of the next call
    });
}
int ldsp_stbank_num_outputs(ldsp_stbank_t q, size_t K, size_t* ncols)
{
    return guard([&] {
        NONNULL(q);
        NONNULL(ncols);
        *ncols = q->num_outputs(K);
    });
}
int ldsp_stbank_execute(ldsp_stbank_t q, const void* x, size_t ldx, size_t K, void* y, size_t ldy, size_t* ncols, int mem,
                        void* stream)
{
    LDSP_RANGE("ldsp_stbank_execute");
    return guard([&] {
        NONNULL(q);
        const size_t N = q->num_outputs(K);
        if (ncols) *ncols = N;
        LDSP_REQUIRE(ldx >= K, "stbank_execute: input row stride below the number of samples");
        if (N > ldy) throw Error(LDSP_ERANGE, "stbank_execute: output row stride below the number of output columns");
        LDSP_REQUIRE(K == 0 || x, "stbank_execute: NULL input");
        LDSP_REQUIRE(N == 0 || y, "stbank_execute: NULL output");
        Call call(*q, mem, x, stream);
        const Exec& e = call.e;
        const size_t C = q->C;
        // a host-memory call reads and writes dense [C][K] and [2 C][N] device images
        // (rows of the caller's images are ldx and ldy samples apart)
        const void* dx = q->stg.dev_in(e, x, K * 4, C, ldx * 4);
        float* dy = (float*)q->stg.dev_out(e, y, 2 * C * N * 4);
        if (K > 0) {
            k::StbankCall c;
            c.x = (const float*)dx;
            c.hist = (const float*)q->hist.in();
            c.hist_out = (float*)q->hist.out();
            c.n = K;
            c.ldx = e.host ? K : ldx;
            c.skip = q->skip();
            c.ncols = N;
            c.ldy = e.host ? N : ldy;
            c.C = (int)C;
            c.D = (int)q->D;
            c.L = (int)q->h.size();
            c.taps = q->dtaps.as<float>();
            c.thr2 = q->thr * q->thr;
            c.y = dy;
            c.level = q->dlevel.as<float>();
            k::stbank(c, e.stream);
            q->hist.flip();
            q->seen += K;
        }
        call.end();
        q->stg.finish(e, y, N * 4, 2 * C, ldy * 4);
    });
}
int ldsp_stbank_get_pilot_level(ldsp_stbank_t q, float* level)
{
    return guard([&] {
        NONNULL(q);
        NONNULL(level);
        std::fill(level, level + q->C, 0.0f);         // before the first call: nothing on the device yet
        q->at_rest([&] { LDSP_HIP(hipMemcpy(level, q->dlevel.p, (size_t)q->C * 4, hipMemcpyDeviceToHost)); });
    });
}
int ldsp_debug_stbank_tile(unsigned int D, unsigned int L, size_t* frames)
{
    return guard([&] {
        NONNULL(frames);
        LDSP_REQUIRE(D >= 1 && D <= (unsigned)k::kStbankMaxD,
                     "stbank: the decimation must lie in 1 .. " + std::to_string(k::kStbankMaxD));
        stbank_check_length(L);
        *frames = (size_t)k::stbank_frames((int)D, (int)L);
    });
}

// ---------------------------------------------------------------- AMBank
static void ambank_check_shape(unsigned int C, unsigned int D, float thr)
{
    LDSP_REQUIRE(C >= 1 && C <= (unsigned)k::kAmbankMaxC,
                 "ambank: the row count must lie in 1 .. " + std::to_string(k::kAmbankMaxC));
    LDSP_REQUIRE(D >= 1 && D <= (unsigned)k::kAmbankMaxD,
                 "ambank: the decimation must lie in 1 .. " + std::to_string(k::kAmbankMaxD));
    LDSP_REQUIRE(thr >= 0.0f, "ambank: the carrier threshold must be >= 0");
}
static void ambank_check_length(unsigned int L)
{
    LDSP_REQUIRE(L >= 1 && L <= (unsigned)k::kAmbankMaxL,
                 "ambank: the prototype length must lie in 1 .. " + std::to_string(k::kAmbankMaxL));
}
// d[j] = (float)((double)h[j] - (double)g[j]): the audio band with the carrier taken out, rounded once
static ldsp_ambank_s* ambank_make(unsigned int C, unsigned int D, float thr, std::vector<float> h, std::vector<float> g)
{
    std::unique_ptr<ldsp_ambank_s> o(new ldsp_ambank_s());
    o->C = C;
    o->D = D;
    o->thr = thr;
    o->d.resize(h.size());
    for (size_t j = 0; j < h.size(); j++) o->d[j] = (float)((double)h[j] - (double)g[j]);
    o->h = std::move(h);
    o->g = std::move(g);
    return o.release();
}
int ldsp_ambank_create(unsigned int C, unsigned int D, double audio, double carrier, unsigned int L, float as,
                       float threshold, ldsp_ambank_t* q)
{
    return guard([&] {
        NONNULL(q);
        ambank_check_shape(C, D, threshold);
        if (audio == 0.0) audio = D == 1 ? 0.45 : 0.5 / (double)D;   // the default audio cut-off
        LDSP_REQUIRE(carrier > 0.0 && carrier < audio && audio <= 0.5,
                     "ambank: the cut-offs must satisfy 0 < carrier < audio <= 0.5 cycles per sample");
        LDSP_REQUIRE(as > 0.0f, "ambank: stop-band attenuation must be > 0");
        if (L == 0) {                                 // the default length
            const double half = std::ceil(2.0 / carrier);
            if (2.0 * half + 1.0 > (double)k::kAmbankMaxL)
                throw Error(LDSP_EUNSUP, "ambank: a default prototype above " + std::to_string(k::kAmbankMaxL) +
                                             " taps is not implemented (carrier cut-off too low)");
            L = 2 * (unsigned)half + 1;
        }
        ambank_check_length(L);
        *q = ambank_make(C, D, threshold, stbank_design(L, audio, as), stbank_design(L, carrier, as));
    });
}
int ldsp_ambank_create_taps(unsigned int C, unsigned int D, const float* h, unsigned int L, const float* g, unsigned int Lg,
                            float threshold, ldsp_ambank_t* q)
{
    return guard([&] {
        NONNULL(q);
        ambank_check_shape(C, D, threshold);
        ambank_check_length(L);
        LDSP_REQUIRE(Lg == L, "ambank: the audio and the carrier prototype must have the same length");
        NONNULL(h);
        NONNULL(g);
        *q = ambank_make(C, D, threshold, std::vector<float>(h, h + L), std::vector<float>(g, g + L));
    });
}
int ldsp_ambank_destroy(ldsp_ambank_t q) { return guard([&] { destroy(q); }); }
int ldsp_ambank_reset(ldsp_ambank_t q)
{
    return guard([&] {
        NONNULL(q);
        q->seen = 0;
        q->at_rest([&] { q->zero_state(q->device); });
    });
}
int ldsp_ambank_get_info(ldsp_ambank_t q, unsigned int* C, unsigned int* D, unsigned int* L, unsigned int* skip)
{
    return guard([&] {
        NONNULL(q);
        if (C) *C = q->C;
        if (D) *D = q->D;
        if (L) *L = (unsigned)q->h.size();
        if (skip) *skip = (unsigned)q->skip();
    });
}
int ldsp_ambank_get_taps(ldsp_ambank_t q, float* h, float* g, float* d)
{
    return guard([&] {
        NONNULL(q);
        if (h) std::copy(q->h.begin(), q->h.end(), h);
        if (g) std::copy(q->g.begin(), q->g.end(), g);
        if (d) std::copy(q->d.begin(), q->d.end(), d);
    });
}
int ldsp_ambank_get_threshold(ldsp_ambank_t q, float* t) { return guard([&] { NONNULL(q); NONNULL(t); *t = q->thr; }); }
int ldsp_ambank_set_threshold(ldsp_ambank_t q, float t)
{
    return guard([&] {
        NONNULL(q);
        LDSP_REQUIRE(t >= 0.0f, "ambank: the carrier threshold must be >= 0");
        q->thr = t;                                   // a kernel argument of the next call
    });
}
int ldsp_ambank_num_outputs(ldsp_ambank_t q, size_t K, size_t* ncols)
{
    return guard([&] {
        NONNULL(q);
        NONNULL(ncols);
        *ncols = q->num_outputs(K);
    });
}
int ldsp_ambank_execute(ldsp_ambank_t q, const void* x, size_t ldx, size_t K, void* y, size_t ldy, size_t* ncols, int mem,
                        void* stream)
{
    LDSP_RANGE("ldsp_ambank_execute");
    return guard([&] {
        NONNULL(q);
        const size_t N = q->num_outputs(K);
        if (ncols) *ncols = N;
        LDSP_REQUIRE(ldx >= K, "ambank_execute: input row stride below the number of samples");
        if (N > ldy) throw Error(LDSP_ERANGE, "ambank_execute: output row stride below the number of output columns");
        LDSP_REQUIRE(K == 0 || x, "ambank_execute: NULL input");
        LDSP_REQUIRE(N == 0 || y, "ambank_execute: NULL output");
        Call call(*q, mem, x, stream);
        const Exec& e = call.e;
        const size_t C = q->C;
        // a host-memory call reads and writes dense [C][K] and [C][N] device images
        // (rows of the caller's images are ldx and ldy samples apart)
        const void* dx = q->stg.dev_in(e, x, K * 8, C, ldx * 8);
        float* dy = (float*)q->stg.dev_out(e, y, C * N * 4);
        if (K > 0) {
            k::AmbankCall c;
            c.x = dx;
            c.hist = q->hist.in();
            c.hist_out = q->hist.out();
            c.n = K;
            c.ldx = e.host ? K : ldx;
            c.skip = q->skip();
            c.ncols = N;
            c.ldy = e.host ? N : ldy;
            c.C = (int)C;
            c.D = (int)q->D;
            c.L = (int)q->h.size();
            c.taps = q->dtaps.as<float>();
            c.thr2 = q->thr * q->thr;
            c.y = dy;
            c.level = q->dlevel.as<float>();
            k::ambank(c, e.stream);
            q->hist.flip();
            q->seen += K;
        }
        call.end();
        q->stg.finish(e, y, N * 4, C, ldy * 4);
    });
}
int ldsp_ambank_get_carrier_level(ldsp_ambank_t q, float* level)
{
    return guard([&] {
        NONNULL(q);
        NONNULL(level);
        std::fill(level, level + q->C, 0.0f);         // before the first call: nothing on the device yet
        q->at_rest([&] { LDSP_HIP(hipMemcpy(level, q->dlevel.p, (size_t)q->C * 4, hipMemcpyDeviceToHost)); });
    });
}
int ldsp_debug_ambank_tile(unsigned int D, unsigned int L, size_t* frames)
{
    return guard([&] {
        NONNULL(frames);
        LDSP_REQUIRE(D >= 1 && D <= (unsigned)k::kAmbankMaxD,
                     "ambank: the decimation must lie in 1 .. " + std::to_string(k::kAmbankMaxD));
        ambank_check_length(L);
        *frames = (size_t)k::ambank_frames((int)D, (int)L);
    });
}

// ---------------------------------------------------------------- SSBBank
static void ssbbank_check_length(unsigned int L)
{
    LDSP_REQUIRE(L >= 1 && L <= (unsigned)k::kSsbbankMaxL,
                 "ssbbank: the prototype length must lie in 1 .. " + std::to_string(k::kSsbbankMaxL));
}
// The shape and the band: hi = 0 stands for 0.5 / D - lo.  Returns hi.
static double ssbbank_check_shape(unsigned int C, unsigned int D, double lo, double hi)
{
    LDSP_REQUIRE(C >= 1 && C <= (unsigned)k::kSsbbankMaxC,
                 "ssbbank: the row count must lie in 1 .. " + std::to_string(k::kSsbbankMaxC));
    LDSP_REQUIRE(D >= 1 && D <= (unsigned)k::kSsbbankMaxD,
                 "ssbbank: the decimation must lie in 1 .. " + std::to_string(k::kSsbbankMaxD));
    if (hi == 0.0) hi = 0.5 / (double)D - lo;         // the default upper edge
    LDSP_REQUIRE(lo > 0.0 && lo < hi && hi <= 0.5 / (double)D,
                 "ssbbank: the band must satisfy 0 < lo < hi <= 0.5 / D cycles per sample");
    return hi;
}
// w = rint(bfo 2^32) mod 2^32 (the product is exact, rint rounds ties to even); 0.5 is the word of -0.5
static std::vector<uint32_t> ssbbank_words(const double* bfo, unsigned int C)
{
    LDSP_REQUIRE(bfo != nullptr, "bfo must not be NULL");
    std::vector<uint32_t> w(C);
    for (unsigned c = 0; c < C; c++) {
        LDSP_REQUIRE(std::isfinite(bfo[c]) && std::fabs(bfo[c]) <= 0.5,
                     "ssbbank: a BFO must lie in -0.5 .. 0.5 cycles per row sample");
        w[c] = (uint32_t)(uint64_t)(int64_t)std::nearbyint(bfo[c] * 4294967296.0);
    }
    return w;
}
static std::vector<int> ssbbank_sides(const int* s, unsigned int C)
{
    LDSP_REQUIRE(s != nullptr, "sideband must not be NULL");
    for (unsigned c = 0; c < C; c++) LDSP_REQUIRE(s[c] == 1 || s[c] == -1, "ssbbank: a sideband is +1 (usb) or -1 (lsb)");
    return std::vector<int>(s, s + C);
}
static ldsp_ssbbank_s* ssbbank_make(unsigned int C, unsigned int D, double lo, double hi, std::vector<float> p,
                                    const double* bfo, const int* sideband)
{
    std::unique_ptr<ldsp_ssbbank_s> o(new ldsp_ssbbank_s());
    o->C = C;
    o->D = D;
    o->lo = lo;
    o->hi = hi;
    o->w = ssbbank_words(bfo, C);
    o->side = ssbbank_sides(sideband, C);
    o->bfo.assign(bfo, bfo + C);
    o->p = std::move(p);
    o->make_taps();
    return o.release();
}
int ldsp_ssbbank_create(unsigned int C, unsigned int D, double lo, double hi, unsigned int L, float as, const double* bfo,
                        const int* sideband, ldsp_ssbbank_t* q)
{
    return guard([&] {
        NONNULL(q);
        hi = ssbbank_check_shape(C, D, lo, hi);
        LDSP_REQUIRE(as > 0.0f, "ssbbank: stop-band attenuation must be > 0");
        if (L != 0) ssbbank_check_length(L);
        (void)ssbbank_words(bfo, C);                  // a value out of range comes before a length not implemented
        (void)ssbbank_sides(sideband, C);
        if (L == 0) {                                 // the default length
            const double half = std::ceil(1.0 / lo);
            if (2.0 * half + 1.0 > (double)k::kSsbbankMaxL)
                throw Error(LDSP_EUNSUP, "ssbbank: a default prototype above " + std::to_string(k::kSsbbankMaxL) +
                                             " taps is not implemented (lo too low)");
            L = 2 * (unsigned)half + 1;
        }
        *q = ssbbank_make(C, D, lo, hi, stbank_design(L, (hi - lo) * 0.5, as), bfo, sideband);
    });
}
int ldsp_ssbbank_create_taps(unsigned int C, unsigned int D, const float* p, unsigned int L, double lo, double hi,
                             const double* bfo, const int* sideband, ldsp_ssbbank_t* q)
{
    return guard([&] {
        NONNULL(q);
        hi = ssbbank_check_shape(C, D, lo, hi);
        ssbbank_check_length(L);
        NONNULL(p);
        *q = ssbbank_make(C, D, lo, hi, std::vector<float>(p, p + L), bfo, sideband);
    });
}
int ldsp_ssbbank_destroy(ldsp_ssbbank_t q) { return guard([&] { destroy(q); }); }
static void ssbbank_restart(ldsp_ssbbank_t q, uint64_t T)
{
    q->seen = T;
    q->at_rest([&] { q->hist.zero(q->hist_bytes(), q->device); });
}
int ldsp_ssbbank_reset(ldsp_ssbbank_t q) { return guard([&] { NONNULL(q); ssbbank_restart(q, 0); }); }
int ldsp_debug_ssbbank_seek(ldsp_ssbbank_t q, uint64_t T) { return guard([&] { NONNULL(q); ssbbank_restart(q, T); }); }
int ldsp_ssbbank_get_info(ldsp_ssbbank_t q, unsigned int* C, unsigned int* D, unsigned int* L, unsigned int* skip)
{
    return guard([&] {
        NONNULL(q);
        if (C) *C = q->C;
        if (D) *D = q->D;
        if (L) *L = (unsigned)q->p.size();
        if (skip) *skip = (unsigned)q->skip();
    });
}
int ldsp_ssbbank_get_band(ldsp_ssbbank_t q, double* lo, double* hi)
{
    return guard([&] {
        NONNULL(q);
        if (lo) *lo = q->lo;
        if (hi) *hi = q->hi;
    });
}
int ldsp_ssbbank_get_taps(ldsp_ssbbank_t q, float* p, float* g)
{
    return guard([&] {
        NONNULL(q);
        if (p) std::copy(q->p.begin(), q->p.end(), p);
        if (g) std::copy(q->g.begin(), q->g.end(), g);
    });
}
int ldsp_ssbbank_get_words(ldsp_ssbbank_t q, uint32_t* w)
{
    return guard([&] {
        NONNULL(q);
        NONNULL(w);
        std::copy(q->w.begin(), q->w.end(), w);
    });
}
int ldsp_ssbbank_get_bfo(ldsp_ssbbank_t q, double* bfo)
{
    return guard([&] {
        NONNULL(q);
        NONNULL(bfo);
        std::copy(q->bfo.begin(), q->bfo.end(), bfo);
    });
}
int ldsp_ssbbank_get_sideband(ldsp_ssbbank_t q, int* sideband)
{
    return guard([&] {
        NONNULL(q);
        NONNULL(sideband);
        std::copy(q->side.begin(), q->side.end(), sideband);
    });
}
// A retune: new taps on the host, and the device tables change only once the
// object's earlier calls have finished with them; on a failure the old lists stay
static void ssbbank_retune(ldsp_ssbbank_t q, const std::function<void()>& change)
{
    std::vector<double> bfo = q->bfo;
    std::vector<uint32_t> w = q->w;
    std::vector<int> side = q->side;
    std::vector<float> g = q->g;
    change();
    try {
        q->make_taps();
        q->at_rest([&] { q->upload_tables(q->device); });
    } catch (...) {
        q->bfo.swap(bfo);
        q->w.swap(w);
        q->side.swap(side);
        q->g.swap(g);
        throw;
    }
}
int ldsp_ssbbank_set_bfo(ldsp_ssbbank_t q, const double* bfo)
{
    return guard([&] {
        NONNULL(q);
        std::vector<uint32_t> w = ssbbank_words(bfo, q->C);
        ssbbank_retune(q, [&] {
            q->w = std::move(w);
            q->bfo.assign(bfo, bfo + q->C);
        });
    });
}
int ldsp_ssbbank_set_sideband(ldsp_ssbbank_t q, const int* sideband)
{
    return guard([&] {
        NONNULL(q);
        std::vector<int> s = ssbbank_sides(sideband, q->C);
        ssbbank_retune(q, [&] { q->side = std::move(s); });
    });
}
int ldsp_ssbbank_num_outputs(ldsp_ssbbank_t q, size_t K, size_t* ncols)
{
    return guard([&] {
        NONNULL(q);
        NONNULL(ncols);
        *ncols = q->num_outputs(K);
    });
}
int ldsp_ssbbank_execute(ldsp_ssbbank_t q, const void* x, size_t ldx, size_t K, void* y, size_t ldy, size_t* ncols, int mem,
                         void* stream)
{
    LDSP_RANGE("ldsp_ssbbank_execute");
    return guard([&] {
        NONNULL(q);
        const size_t N = q->num_outputs(K);
        if (ncols) *ncols = N;
        LDSP_REQUIRE(ldx >= K, "ssbbank_execute: input row stride below the number of samples");
        if (N > ldy) throw Error(LDSP_ERANGE, "ssbbank_execute: output row stride below the number of output columns");
        LDSP_REQUIRE(K == 0 || x, "ssbbank_execute: NULL input");
        LDSP_REQUIRE(N == 0 || y, "ssbbank_execute: NULL output");
        Call call(*q, mem, x, stream);
        const Exec& e = call.e;
        const size_t C = q->C;
        // a host-memory call reads and writes dense [C][K] and [C][N] device images
        // (rows of the caller's images are ldx and ldy samples apart)
        const void* dx = q->stg.dev_in(e, x, K * 8, C, ldx * 8);
        float* dy = (float*)q->stg.dev_out(e, y, C * N * 4);
        if (K > 0) {
            k::SsbbankCall c;
            c.x = dx;
            c.hist = q->hist.in();
            c.hist_out = q->hist.out();
            c.n = K;
            c.ldx = e.host ? K : ldx;
            c.skip = q->skip();
            c.ncols = N;
            c.ldy = e.host ? N : ldy;
            c.col0 = q->next_column();
            c.C = (int)C;
            c.D = (int)q->D;
            c.L = (int)q->p.size();
            c.taps = q->dtaps.as<float>();
            c.words = q->dwords.as<uint32_t>();
            c.y = dy;
            k::ssbbank(c, e.stream);
            q->hist.flip();
            q->seen += K;
        }
        call.end();
        q->stg.finish(e, y, N * 4, C, ldy * 4);
    });
}
int ldsp_debug_ssbbank_tile(unsigned int D, unsigned int L, size_t* frames)
{
    return guard([&] {
        NONNULL(frames);
        LDSP_REQUIRE(D >= 1 && D <= (unsigned)k::kSsbbankMaxD,
                     "ssbbank: the decimation must lie in 1 .. " + std::to_string(k::kSsbbankMaxD));
        ssbbank_check_length(L);
        *frames = (size_t)k::ssbbank_frames((int)D, (int)L);
    });
}

// ---------------------------------------------------------------- Spectrogram
static void spgram_check_shape(unsigned int N, unsigned int W, unsigned int d, unsigned int A)
{
    LDSP_REQUIRE(N >= 1 && (N & (N - 1)) == 0, "spgram: nfft must be a power of two");
    if (N < 256 || N > 4096) throw Error(LDSP_EUNSUP, "spgram: nfft below 256 or above 4096 is not implemented");
    LDSP_REQUIRE(W >= 1 && W <= N, "spgram: the window length must lie in 1 .. nfft");
    LDSP_REQUIRE(d >= 1, "spgram: the delay must be at least 1");
    if (d > W) throw Error(LDSP_EUNSUP, "spgram: a delay above the window length is not implemented");
    LDSP_REQUIRE(A >= 1, "spgram: average must be at least 1");
}
static ldsp_spgram_s* spgram_make(unsigned int N, unsigned int W, unsigned int d, unsigned int A, std::vector<float> w)
{
    std::unique_ptr<ldsp_spgram_s> o(new ldsp_spgram_s());
    o->N = N;
    o->W = W;
    o->d = d;
    o->A = A;
    o->w = std::move(w);
    return o.release();
}
// the named windows: double, normalised to sum w^2 = 1 in double, rounded once
static std::vector<float> spgram_window(int wtype, unsigned int W)
{
    std::vector<double> v(W);
    for (unsigned i = 0; i < W; i++) {
        const double t = W > 1 ? (double)i / (double)(W - 1) : 0.0;
        const double c1 = cos(2.0 * M_PI * t), c2 = cos(4.0 * M_PI * t), c3 = cos(6.0 * M_PI * t);
        switch (wtype) {
        case LDSP_WIN_RECT: v[i] = 1.0; break;
        case LDSP_WIN_HANN: v[i] = 0.5 - 0.5 * c1; break;
        case LDSP_WIN_HAMMING: v[i] = 0.53836 - 0.46164 * c1; break;
        default: v[i] = 0.35875 - 0.48829 * c1 + 0.14128 * c2 - 0.01168 * c3; break;
        }
    }
    if (W == 1) v[0] = 1.0;
    double e = 0.0;
    for (double a : v) e += a * a;
    const double g = 1.0 / sqrt(e);
    std::vector<float> w(W);
    for (unsigned i = 0; i < W; i++) w[i] = (float)(v[i] * g);
    return w;
}
int ldsp_spgram_create(unsigned int nfft, int wtype, unsigned int W, unsigned int d, unsigned int A, ldsp_spgram_t* q)
{
    return guard([&] {
        NONNULL(q);
        spgram_check_shape(nfft, W, d, A);
        LDSP_REQUIRE(wtype >= LDSP_WIN_RECT && wtype <= LDSP_WIN_BLACKMANHARRIS, "spgram: unknown window type");
        *q = spgram_make(nfft, W, d, A, spgram_window(wtype, W));
    });
}
int ldsp_spgram_create_window(unsigned int nfft, const float* w, unsigned int W, unsigned int d, unsigned int A,
                              ldsp_spgram_t* q)
{
    return guard([&] {
        NONNULL(q);
        spgram_check_shape(nfft, W, d, A);
        NONNULL(w);
        *q = spgram_make(nfft, W, d, A, std::vector<float>(w, w + W));
    });
}
int ldsp_spgram_destroy(ldsp_spgram_t q) { return guard([&] { destroy(q); }); }
int ldsp_spgram_reset(ldsp_spgram_t q)
{
    return guard([&] {
        NONNULL(q);
        q->seen = 0;
        q->nacc = 0;
        q->at_rest([&] {
            q->zero_stream(q->device);
            q->zero_psd(q->device);
        });
    });
}
int ldsp_spgram_clear(ldsp_spgram_t q)
{
    return guard([&] {
        NONNULL(q);
        q->nacc = 0;
        q->at_rest([&] { q->zero_psd(q->device); });
    });
}
int ldsp_spgram_get_info(ldsp_spgram_t q, unsigned int* nfft, unsigned int* W, unsigned int* d, unsigned int* A,
                         uint64_t* samples, uint64_t* transforms)
{
    return guard([&] {
        NONNULL(q);
        if (nfft) *nfft = q->N;
        if (W) *W = q->W;
        if (d) *d = q->d;
        if (A) *A = q->A;
        if (samples) *samples = q->seen;
        if (transforms) *transforms = q->nacc;
    });
}
int ldsp_spgram_get_window(ldsp_spgram_t q, float* w)
{
    return guard([&] {
        NONNULL(q);
        NONNULL(w);
        std::copy(q->w.begin(), q->w.end(), w);
    });
}
int ldsp_spgram_num_outputs(ldsp_spgram_t q, size_t n, size_t* ntransforms, size_t* nrows)
{
    return guard([&] {
        NONNULL(q);
        if (ntransforms) *ntransforms = q->transforms(n);
        if (nrows) *nrows = q->rows(n);
    });
}
// One piece of a call: launches, then the host-side state moves on.
static void spgram_piece(ldsp_spgram_s* q, const void* dx, size_t n, float* dy, size_t dld, hipStream_t stream,
                         bool iq16)
{
    const unsigned N = q->N;
    const bool blocked = k::spgram_blocked(q->A);
    const size_t A = blocked ? (size_t)k::kSpgramBlock : (size_t)q->A;   // transforms per row of the main kernel
    const uint64_t s0 = q->seen / q->d, s1 = (q->seen + n) / q->d;
    const size_t nt = (size_t)(s1 - s0);
    const size_t nb = (size_t)(s1 / A - s0 / A);                         // its finished rows: blocks when blocked
    k::SpgramCall c;
    c.x = dx;
    c.hist = q->hist.in();
    c.hist_out = q->hist.out();
    c.n = n;
    c.A = A;
    c.a0 = (size_t)(s0 % A);
    c.nt = nt;
    c.ld = blocked ? N : dld;
    c.base = (long long)((s0 + 1) * q->d - q->seen) - (long long)q->W;
    c.W = (int)q->W;
    c.d = (int)q->d;
    c.win = q->dwin.as<float>();
    c.tw = q->dtw.p;
    c.carry_in = (float*)q->carry.in();
    c.carry_out = (float*)q->carry.out();
    c.scale = blocked ? 1.0f : 1.0f / (float)q->A;
    c.y = blocked ? (float*)q->blk.ensure(std::max<size_t>(nb, 1) * N * 4, q->device) : dy;
    const size_t runs = k::spgram_runs((int)N, c.A, c.a0, nt, nullptr);
    c.part = (float*)q->part.ensure(std::max<size_t>(runs, 1) * N * 4, q->device);
    c.psd = q->dpsd.as<double>();
    c.iq16 = iq16;
    k::spgram((int)N, c, stream);
    q->hist.flip();
    // the unfinished row (block) moved to the other buffer if the piece left one behind
    if (nt > 0 && s1 % A != 0) q->carry.flip();
    if (blocked && nb > 0) {
        const size_t M = q->A / A, c0 = (size_t)((s0 / A) % M);
        k::spgram_rows((int)N, c.y, nb, M, c0, (float*)q->rcarry.in(), (float*)q->rcarry.out(), q->A, dy, dld, stream);
        if ((c0 + nb) % M != 0) q->rcarry.flip();
    }
    q->seen += n;
    q->nacc += nt;
}
// iq16: x is n int16 (I, Q) pairs (bytes_to_iq's input), converted by the kernel's loads
static int spgram_execute(ldsp_spgram_t q, const void* x, size_t n, float* y, size_t ld, size_t* nrows, int mem,
                          void* stream, bool iq16)
{
    return guard([&] {
        NONNULL(q);
        const size_t K = q->rows(n);
        if (nrows) *nrows = K;
        LDSP_REQUIRE(n == 0 || x, "spgram_execute: NULL input");
        checked_mem(mem);                      // (reported before the stride)
        LDSP_REQUIRE(!y || ld >= q->N, "spgram_execute: row stride below nfft");
        Call call(*q, mem, x, stream);
        const Exec& e = call.e;
        const unsigned N = q->N;
        // a host-memory call computes into a dense [K][N] device image
        // (rows of the caller's image are ld floats apart)
        const bool rows_out = y != nullptr && K > 0;
        const size_t dld = e.host ? N : ld;
        const size_t xsz = iq16 ? 4 : 8;      // bytes per input sample
        const void* dx = q->stg.dev_in(e, x, n * xsz);
        float* const dy0 = rows_out ? (float*)q->stg.dev_out(e, y, K * (size_t)N * 4) : nullptr;
        float* dy = dy0;
        // a blocked average is taken in pieces of at most kSpgramMaxBlocks blocks
        // (the block sums go through memory); the cut of a stream changes no bit
        const size_t piece = k::spgram_blocked(q->A)
                                 ? (size_t)q->d * k::kSpgramBlock * k::kSpgramMaxBlocks - (size_t)q->d * k::kSpgramBlock
                                 : n;
        for (size_t off = 0; off < n;) {
            const size_t m = std::min(n - off, piece);
            const size_t done = q->rows(m);
            spgram_piece(q, (const char*)dx + off * xsz, m, dy, dld, e.stream, iq16);
            if (dy) dy += done * dld;
            off += m;
        }
        call.end();
        q->stg.finish(e, y, (size_t)N * 4, rows_out ? K : 0, ld * 4);
    });
}
int ldsp_spgram_execute(ldsp_spgram_t q, const void* x, size_t n, float* y, size_t ld, size_t* nrows, int mem,
                        void* stream)
{
    LDSP_RANGE("ldsp_spgram_execute");
    return spgram_execute(q, x, n, y, ld, nrows, mem, stream, false);
}
int ldsp_spgram_execute_iq16(ldsp_spgram_t q, const void* x, size_t n, float* y, size_t ld, size_t* nrows, int mem,
                             void* stream)
{
    LDSP_RANGE("ldsp_spgram_execute_iq16");
    return spgram_execute(q, x, n, y, ld, nrows, mem, stream, true);
}
int ldsp_spgram_get_psd(ldsp_spgram_t q, double* psd, uint64_t* transforms)
{
    return guard([&] {
        NONNULL(q);
        NONNULL(psd);
        if (transforms) *transforms = q->nacc;
        std::fill(psd, psd + q->N, 0.0);
        if (q->nacc == 0) return;
        q->at_rest([&] {
            LDSP_HIP(hipMemcpy(psd, q->dpsd.p, (size_t)q->N * 8, hipMemcpyDeviceToHost));
            const double s = (double)q->nacc;
            for (unsigned k = 0; k < q->N; k++) psd[k] /= s;
        });
    });
}
int ldsp_debug_spgram_tile(unsigned int nfft, size_t* transforms)
{
    return guard([&] {
        NONNULL(transforms);
        spgram_check_shape(nfft, 1, 1, 1);
        *transforms = (size_t)k::spgram_tile((int)nfft);
    });
}

// ---------------------------------------------------------------- FMStereo
int ldsp_fmstereo_create(float iq_rate, float pcm_rate, ldsp_fmstereo_t* q)
{
    return guard([&] {
        NONNULL(q);
        LDSP_REQUIRE(iq_rate > 0.0f && pcm_rate > 0.0f, "fmstereo: rates must be > 0");
        const float rate = pcm_rate / iq_rate;
        if (rate > 1.0f)
            throw Error(LDSP_EUNSUP, "fmstereo: pcm_rate > iq_rate (the reference drops the samples of inputs that "
                                     "produce two outputs, demod.hpp:45-47; not reproduced)");
        std::unique_ptr<ldsp_fmstereo_s> o(new ldsp_fmstereo_s());
        o->iq_rate = iq_rate;
        o->pcm_rate = pcm_rate;
        // demod.hpp:19-31: 75 us de-emphasis (double arithmetic stored as float)
        float a[2], b[1];
        a[0] = 1.0;
        a[1] = -exp(-1.0 / (75.0E-6 * iq_rate));
        b[0] = 1.0 + a[1];
        ok(ldsp_freqdem_create(4.0f, &o->dem));
        for (int c = 0; c < 2; c++) {
            ok(ldsp_iirfilt_create_tf(b, 1, a, 2, 0, &o->emph[c]));
            ok(ldsp_iirfilt_set_mode(o->emph[c], LDSP_MODE_EXACT));
            ok(ldsp_resamp_create_default(rate, 0, &o->aud[c]));
        }
        o->table = nco_table();
        o->st.theta = 0;
        o->st.dtheta = 0;
        o->st.pe = 0.0f;           // uninitialised member in the reference (demod.hpp:13)
        o->st.alpha = 0.1f;        // nco_crcf_create: PLL bandwidth 0.1
        o->st.beta = sqrtf(0.1f);
        *q = o.release();
    });
}
int ldsp_fmstereo_destroy(ldsp_fmstereo_t q) { return guard([&] { destroy(q); }); }   // and its stages
int ldsp_fmstereo_reset(ldsp_fmstereo_t q)
{
    return guard([&] {
        NONNULL(q);
        for (int c = 0; c < 2; c++) ok(ldsp_resamp_reset(q->aud[c]));   // demod.hpp:34-37: only the resamplers
    });
}
int ldsp_fmstereo_num_outputs(ldsp_fmstereo_t q, size_t n, size_t* nout)
{
    return guard([&] {
        NONNULL(q);
        NONNULL(nout);
        size_t k = 0;
        ok(ldsp_resamp_num_outputs(q->aud[0], n, &k));
        *nout = 2 * k;
    });
}
int ldsp_fmstereo_get_state(ldsp_fmstereo_t q, uint32_t* theta, uint32_t* dtheta, float* pe)
{
    return guard([&] {
        NONNULL(q);
        q->at_rest([&] { LDSP_HIP(hipMemcpy(&q->st, q->dst.p, sizeof(q->st), hipMemcpyDeviceToHost)); });
        if (theta) *theta = q->st.theta;
        if (dtheta) *dtheta = q->st.dtheta;
        if (pe) *pe = q->st.pe;
    });
}
int ldsp_fmstereo_execute(ldsp_fmstereo_t q, const void* x, size_t n, void* y, size_t cap, size_t* nout, int mem,
                          void* stream)
{
    LDSP_RANGE("ldsp_fmstereo_execute");
    return guard([&] {
        NONNULL(q);
        size_t k = 0;
        ok(ldsp_resamp_num_outputs(q->aud[0], n, &k));
        if (nout) *nout = 2 * k;
        if (2 * k > cap) throw Error(LDSP_ERANGE, "fmstereo_execute: output capacity too small");
        LDSP_REQUIRE(n == 0 || x, "fmstereo_execute: NULL input");
        LDSP_REQUIRE(k == 0 || y, "fmstereo_execute: NULL output");
        Call call(*q, mem, x, stream);
        const Exec& e = call.e;
        const void* dx = q->stg.dev_in(e, x, n * 8);
        float* dy = (float*)q->stg.dev_out(e, y, 2 * k * 4);
        if (n > 0) {
            float* sd = (float*)q->sbuf.ensure(n * 4, q->device);
            ok(ldsp_freqdem_demodulate(q->dem, dx, n, sd, LDSP_MEM_DEVICE, e.stream));
            float* l = (float*)q->lr[0].ensure(n * 4, q->device);
            float* r = (float*)q->lr[1].ensure(n * 4, q->device);
            k::fm_pll(sd, n, q->dst.as<k::FmState>(), q->dtab.as<float>(), l, r, e.stream);
            float* outs[2];
            for (int c = 0; c < 2; c++) {
                float* de = (float*)q->le[c].ensure(n * 4, q->device);
                ok(ldsp_iirfilt_execute(q->emph[c], c ? r : l, n, de, LDSP_MEM_DEVICE, e.stream));
                outs[c] = (float*)q->out[c].ensure(std::max<size_t>(k, 1) * 4, q->device);
                size_t kc = 0;
                ok(ldsp_resamp_execute(q->aud[c], de, n, outs[c], k, &kc, LDSP_MEM_DEVICE, e.stream));
                LDSP_REQUIRE(kc == k, "fmstereo: resampler output counts diverged");
            }
            k::interleave2(outs[0], outs[1], k, dy, e.stream);
        }
        call.end();
        q->stg.finish(e, y, 2 * k * 4);
    });
}

// ------------------------------------------------------- many-calls (batch.hpp)
// C independent objects of one class, one call each on the same stream, with
// one launch per kernel for all of them: every object's execute runs with the
// recorder active (its host bookkeeping exactly as for a single call), then the
// recorded work is issued with the launches of objects that run the same
// kernel on the same grid merged (blockIdx.y = object).  Device memory only;
// the objects must be distinct.
// `batchable(c)`: object c's call takes a path whose every kernel has a merged
// form; otherwise the objects run one after another (the same bits, C times the
// launches) -- e.g. exact-mode transfer-function IIR filters, single-sideband AmpModems.
extern "C++" {
template <class T, class B, class F>
static int run_many(T* const* q, int C, void* stream, B&& batchable, F&& one)
{
    return guard([&] {
        LDSP_REQUIRE(q != nullptr && C >= 1 && C <= 4096, "many: 1 .. 4096 objects");
        for (int c = 0; c < C; c++) {
            LDSP_REQUIRE(q[c] != nullptr, "many: NULL object");
            for (int c2 = 0; c2 < c; c2++) LDSP_REQUIRE(q[c2] != q[c], "many: the objects must be distinct");
        }
        bool all = true;
        for (int c = 0; c < C; c++) all = all && batchable(c);
        if (!all) {
            for (int c = 0; c < C; c++) ok(one(c));
            return;
        }
        BatchRecorder rec(C, (hipStream_t)stream);
        int rc = LDSP_OK;
        std::string err;
        for (int c = 0; c < C && rc == LDSP_OK; c++) {
            rec.channel(c);
            rc = one(c);
            if (rc != LDSP_OK) err = g_last_error;
        }
        rec.flush();                         // every object whose host state advanced gets its device work
        if (rc != LDSP_OK) throw Error(rc, err);
    });
}
} // extern "C++"

int ldsp_agc_execute_many(ldsp_agc_t* q, const void* const* x, size_t n, void* const* y, int C, void* stream)
{
    LDSP_RANGE("ldsp_agc_execute_many");
    return run_many(q, C, stream, [](int) { return true; }, [&](int c) {
        return ldsp_agc_execute(q[c], x[c], n, y[c], nullptr, LDSP_MEM_DEVICE, stream);
    });
}

int ldsp_ampmodem_demodulate_many(ldsp_ampmodem_t* q, const void* const* x, size_t n, void* const* y, int C,
                                  void* stream)
{
    LDSP_RANGE("ldsp_ampmodem_demodulate_many");
    return run_many(q, C, stream, [&](int c) { return q[c]->type == 0; }, [&](int c) {
        return ldsp_ampmodem_demodulate(q[c], x[c], n, y[c], LDSP_MEM_DEVICE, stream);
    });
}

int ldsp_iirfilt_execute_many(ldsp_iirfilt_t* q, const void* const* x, size_t n, void* const* y, int C, void* stream)
{
    LDSP_RANGE("ldsp_iirfilt_execute_many");
    return run_many(q, C, stream, [&](int c) {
        const IirObj::Path p = q[c]->path_for(n);
        // exact SOS cascades: k_iir_sect, one workgroup per (object, component)
        const bool sect = p == IirObj::kSeq && k::iir_seq_kernel(q[c]->desc()).sect_tile != 0;
        return p == IirObj::kSpec || p == IirObj::kModal || sect;
    }, [&](int c) {
        return ldsp_iirfilt_execute(q[c], x[c], n, y[c], LDSP_MEM_DEVICE, stream);
    });
}

int ldsp_iirfilt_resamp_execute_many(ldsp_iirfilt_t* q, ldsp_resamp_t* rs, const void* const* x, size_t n,
                                     void* const* y, size_t cap, size_t* nout, int C, void* stream)
{
    LDSP_RANGE("ldsp_iirfilt_resamp_execute_many");
    if (q == nullptr || rs == nullptr || C < 1 || C > 4096) {
        set_last_error("many: 1 .. 4096 objects, filters and resamplers both given");
        return LDSP_EINVAL;
    }
    for (int c = 0; c < C; c++)
        if (rs[c] == nullptr) {
            set_last_error("many: NULL resampler");
            return LDSP_EINVAL;
        }
    for (int c = 0; c < C; c++)                  // the resamplers must be distinct too
        for (int c2 = 0; c2 < c; c2++)
            if (rs[c] == rs[c2]) {
                set_last_error("many: the objects must be distinct");
                return LDSP_EINVAL;
            }
    return run_many(q, C, stream, [&](int c) {       // the fused pass (ldsp_iirfilt_resamp_execute)
        return rs && rs[c] && q[c]->cplx == rs[c]->cplx && q[c]->path_for(n) == IirObj::kModal &&
               rs[c]->sub_len >= 2 && rs[c]->sub_len - 1 <= 1024u;
    }, [&](int c) {
        return ldsp_iirfilt_resamp_execute(q[c], rs[c], x[c], n, y[c], cap, nout ? nout + c : nullptr,
                                           LDSP_MEM_DEVICE, stream);
    });
}

// ------------------------------------------------------- page-locked host pool
// Blocks are whole 64 KB multiples; a request takes the smallest free block that
// fits and is at most twice its size.  Freed blocks are cached up to kCacheMax
// (hipHostFree beyond it); at most kLiveMax is handed out at a time.
namespace {
struct HostPool {
    static constexpr size_t kCacheMax = (size_t)256 << 20, kLiveMax = (size_t)1 << 30;
    std::mutex mu;
    std::multimap<size_t, void*> free;
    std::map<void*, size_t> live;
    size_t cached = 0, out = 0;
};
HostPool& host_pool()
{
    static HostPool* p = new HostPool();    // never destroyed: frees can come at interpreter teardown
    return *p;
}
} // namespace

int ldsp_host_alloc(size_t bytes, void** p)
{
    return guard([&] {
        LDSP_REQUIRE(p != nullptr, "host_alloc: NULL output pointer");
        *p = nullptr;
        const size_t want = (std::max<size_t>(bytes, 1) + 65535) & ~(size_t)65535;
        HostPool& hp = host_pool();
        void* b = nullptr;
        size_t sz = want;
        {
            std::lock_guard<std::mutex> lk(hp.mu);
            auto it = hp.free.lower_bound(want);
            // the limit counts the block actually handed out (a cached block may be up to 2x want)
            if (it != hp.free.end() && it->first <= 2 * want && hp.out + it->first <= HostPool::kLiveMax) {
                b = it->second;
                sz = it->first;
                hp.cached -= sz;
                hp.free.erase(it);
                hp.live[b] = sz;
                hp.out += sz;
                *p = b;
                return;
            }
            if (hp.out + want > HostPool::kLiveMax) throw Error(LDSP_ENOMEM, "host_alloc: page-locked pool exhausted");
            hp.out += want;                  // reserved while the allocation runs outside the lock
        }
        if (hipHostMalloc(&b, want, hipHostMallocPortable) != hipSuccess || !b) {
            (void)hipGetLastError();
            std::lock_guard<std::mutex> lk(hp.mu);
            hp.out -= want;
            throw Error(LDSP_ENOMEM, "host_alloc: hipHostMalloc failed");
        }
        std::lock_guard<std::mutex> lk(hp.mu);
        hp.live[b] = sz;
        *p = b;
    });
}

int ldsp_host_free(void* p)
{
    return guard([&] {
        if (!p) return;
        HostPool& hp = host_pool();
        std::vector<void*> evict;            // hipHostFree may synchronise the device: never under the lock
        {
            std::lock_guard<std::mutex> lk(hp.mu);
            auto it = hp.live.find(p);
            LDSP_REQUIRE(it != hp.live.end(), "host_free: not a block of ldsp_host_alloc");
            const size_t sz = it->second;
            hp.live.erase(it);
            hp.out -= sz;
            hp.free.emplace(sz, p);
            hp.cached += sz;
            while (hp.cached > HostPool::kCacheMax && !hp.free.empty()) {
                auto big = std::prev(hp.free.end());
                hp.cached -= big->first;
                evict.push_back(big->second);
                hp.free.erase(big);
            }
        }
        for (void* b : evict) (void)hipHostFree(b);
    });
}

int ldsp_debug_host_pools(size_t* total, size_t* idle)
{
    return guard([&] {
        PoolList& l = pool_list();
        std::lock_guard<std::mutex> lk(l.mu);
        size_t f = 0;
        for (const auto& v : l.free) f += v.size();
        if (total) *total = l.total;
        if (idle) *idle = f;
    });
}

// ---------------------------------------------------------------- bytes_to_iq
int ldsp_bytes_to_iq(const void* in, size_t nbytes, void* y, int mem, void* stream)
{
    static std::mutex mu;
    static std::vector<std::unique_ptr<Staging>> stgs;   // per device, host-memory calls only
    return guard([&] {
        const size_t n = nbytes / 4;
        LDSP_REQUIRE(n == 0 || (in && y), "bytes_to_iq: NULL buffer");
        // no object: a transient one binds to the buffer's device and leaves nothing to order
        struct Unbound : DevObj {
            void bind(int) {}
        } none;
        Call call(none, mem, in, stream, false);
        const Exec& e = call.e;
        const int dev = e.device;
        std::unique_lock<std::mutex> lk(mu, std::defer_lock);
        if (e.host) lk.lock();   // the staging buffers are shared by host-memory calls
        if ((int)stgs.size() <= dev) stgs.resize(dev + 1);
        if (!stgs[dev]) stgs[dev].reset(new Staging());
        Staging& stg = *stgs[dev];
        const void* dx = stg.dev_in(e, in, n * 4);
        void* dy = stg.dev_out(e, y, n * 8);
        k::bytes_to_iq(dx, dy, n, e.stream);
        stg.finish(e, y, n * 8);
    });
}

} // extern "C"
