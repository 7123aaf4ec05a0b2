// liquiddsp_module.cpp -- the pybind11 module `liquiddsp`: same class names,
// constructor keywords, defaults, properties and __call__ semantics as the
// reference module (colbyAtCRI/python-liquiddsp src/wrapper.cpp:10-273), bound
// to the MI355X C ABI (include/ldsp.h) instead of liquid-dsp.
//
// Array handling (reference src/liquiddsp.hpp:16-20 array_to_ptr):
//  * numpy / lists / other dtypes are force-cast to contiguous complex64 /
//    float32 (the reference read strided views as if contiguous; this module
//    copies them), staged to the GPU, processed, and a new
//    numpy array is returned.
//  * a torch tensor on a ROCm device is processed in place on the device,
//    enqueued on torch's current stream, and a new device tensor is returned
//    (no host round trip; this is how chains stay resident in HBM).
// The GIL is released while a call waits for the GPU.
#include <pybind11/complex.h>
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cmath>
#include <complex>
#include <cstdio>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/ldsp.h"

namespace py = pybind11;
using cf = std::complex<float>;

namespace {

// ------------------------------------------------------------------ errors
void check(int rc)
{
    if (rc == LDSP_OK) return;
    const std::string msg = ldsp_last_error();
    if (rc == LDSP_EINVAL || rc == LDSP_ERANGE) throw py::value_error(msg);
    if (rc == LDSP_EUNSUP) {
        PyErr_SetString(PyExc_NotImplementedError, msg.c_str());
        throw py::error_already_set();
    }
    throw std::runtime_error(msg);
}

// ------------------------------------------------------------------ torch interop
py::object& torch_mod()
{
    static py::object t = py::module_::import("torch");
    return t;
}

bool is_device_tensor(const py::handle& o)
{
    if (!py::hasattr(o, "is_cuda") || !py::hasattr(o, "data_ptr")) return false;
    return o.attr("is_cuda").cast<bool>();
}

void* tptr(const py::object& t) { return reinterpret_cast<void*>(t.attr("data_ptr")().cast<uintptr_t>()); }

// ------------------------------------------------------------------ the call scaffold
// Every call is: build the input (in_1d / in_rows), ask the C ABI for the
// output size, allocate (make_out), invoke.

// One owner for every C-ABI handle: move-only, destroys on destruction; it
// stands for the handle wherever a C function takes one.
template <typename H, int (*Destroy)(H)>
class Handle {
    H h = nullptr;

public:
    Handle() = default;
    Handle(Handle&& o) noexcept : h(o.h) { o.h = nullptr; }
    Handle& operator=(Handle&& o) noexcept
    {
        std::swap(h, o.h);      // o destroys what this held
        return *this;
    }
    ~Handle() { if (h) Destroy(h); }
    H get() const { return h; }
    operator H() const { return h; }
    H* out() { return &h; }     // for the create functions
};

// float s; check(get(q, &s)); return s;
template <typename T, typename Q, typename G>
T get_value(G get, const Q& q)
{
    T v;
    check(get(q, &v));
    return v;
}

// The element kinds of inputs and results
enum class Kind { f32, c64, i16, u8, i32, i8 };
constexpr Kind kind_of(bool cplx) { return cplx ? Kind::c64 : Kind::f32; }
const char* torch_name(Kind k)
{
    if (k == Kind::i32) return "int32";
    if (k == Kind::i8) return "int8";
    return k == Kind::c64 ? "complex64" : (k == Kind::f32 ? "float32" : (k == Kind::i16 ? "int16" : "uint8"));
}
size_t kind_size(Kind k)
{
    if (k == Kind::i32) return 4;
    if (k == Kind::i8) return 1;
    return k == Kind::c64 ? 8 : (k == Kind::f32 ? 4 : (k == Kind::i16 ? 2 : 1));
}
py::dtype np_dtype(Kind k)
{
    if (k == Kind::i32) return py::dtype::of<int32_t>();
    if (k == Kind::i8) return py::dtype::of<int8_t>();
    return k == Kind::c64 ? py::dtype::of<cf>()
                          : (k == Kind::f32 ? py::dtype::of<float>()
                                            : (k == Kind::i16 ? py::dtype::of<int16_t>() : py::dtype::of<uint8_t>()));
}
// The dtype dispatch of Delay and HilbertTransform: complex64 or float32, false for anything else
bool kind_from_dtype(const py::handle& x, Kind* k)
{
    py::object tp = py::getattr(x, "dtype");
    const bool dev = is_device_tensor(x);
    for (Kind c : {Kind::c64, Kind::f32})
        if (tp.equal(dev ? py::object(torch_mod().attr(torch_name(c))) : py::object(py::dtype(torch_name(c))))) {
            *k = c;
            return true;
        }
    return false;
}

// One call's input where the call reads it: n samples at ptr (a row image: n
// per row, rows ld samples apart), on the device (with the stream and device
// of the tensor) or on the host.
struct CallIn {
    py::object keep;    // whatever owns the memory, kept alive for the call
    const void* ptr = nullptr;
    size_t n = 0, ld = 0;
    bool dev = false;
    void* stream = nullptr;
    py::object device;
};

// A device tensor as a call's input: its device, checked against the current
// one -- libldsp binds an object to the current HIP device on first use and
// launches there: a tensor on another device would hand it foreign pointers --
// and torch's current stream on it.
enum class DevCheck { none, brief, full };
void on_device(CallIn& in, const py::object& t, DevCheck chk)
{
    py::object& torch = torch_mod();
    in.device = t.attr("device");
    if (chk != DevCheck::none) {
        const int tdev = in.device.attr("index").cast<int>();
        const int cur = torch.attr("cuda").attr("current_device")().cast<int>();
        if (tdev != cur && chk == DevCheck::brief) throw py::value_error("input tensor is not on the current device");
        if (tdev != cur)
            throw py::value_error("input tensor is on cuda:" + std::to_string(tdev) + " but the current device is cuda:" +
                                  std::to_string(cur) + " (call under torch.cuda.device(" + std::to_string(tdev) + "))");
    }
    in.keep = t;
    in.ptr = tptr(t);
    in.dev = true;
    in.stream = reinterpret_cast<void*>(
        torch.attr("cuda").attr("current_stream")(in.device).attr("cuda_stream").cast<uintptr_t>());
}

using carr = py::array_t<cf, py::array::c_style | py::array::forcecast>;
using farr = py::array_t<float, py::array::c_style | py::array::forcecast>;

// x as a contiguous host array of kind k (force-cast)
py::array host_in(const py::handle& x, Kind k)
{
    py::array a = k == Kind::c64 ? py::array(carr::ensure(x)) : py::array(farr::ensure(x));
    if (!a) throw py::error_already_set();
    return a;
}
py::object dev_cast(const py::handle& x, Kind k)
{
    py::object want = torch_mod().attr(torch_name(k));
    py::object t = py::reinterpret_borrow<py::object>(x);
    return py::object(t.attr("dtype")).equal(want) ? t : py::object(t.attr("to")(want));
}

// A 1-D input: a device tensor as it is, anything else force-cast, both
// flattened.  Kind::i16 is the input of the from_bytes / write_bytes methods:
// interleaved int16 (I, Q) pairs as raw bytes -- bytes-like / an int16 or uint8
// numpy array (host) or an int16 / uint8 device tensor.  n then counts whole
// pairs: trailing 1-3 bytes are dropped, as bytes_to_iq does (utility.hpp:65
// rounds size / 4 down).
CallIn in_1d(const py::handle& x, Kind k)
{
    CallIn in;
    if (k == Kind::i16 && is_device_tensor(x)) {
        py::object t = py::reinterpret_borrow<py::object>(x).attr("reshape")(-1).attr("contiguous")();
        on_device(in, t, DevCheck::brief);
        in.n = t.attr("numel")().cast<size_t>() * t.attr("element_size")().cast<size_t>() / 4;
        if (reinterpret_cast<uintptr_t>(in.ptr) % 4) {   // a view at an odd offset: the kernels read 4-byte pairs
            in.keep = t.attr("clone")();
            in.ptr = tptr(in.keep);
        }
    } else if (k == Kind::i16) {
        py::object o = py::reinterpret_borrow<py::object>(x);
        if (py::isinstance<py::array>(o)) o = py::module_::import("numpy").attr("ascontiguousarray")(o);
        py::buffer_info bi = py::reinterpret_borrow<py::buffer>(o).request();
        in.ptr = bi.ptr;
        in.n = (size_t)bi.size * (size_t)bi.itemsize / 4;
        in.keep = o;
    } else if (is_device_tensor(x)) {
        py::object t = dev_cast(x, k).attr("reshape")(-1).attr("contiguous")();
        on_device(in, t, DevCheck::full);
        in.n = t.attr("numel")().cast<size_t>();
    } else {
        py::array a = host_in(x, k);
        in.ptr = a.data();
        in.n = (size_t)a.size();
        in.keep = std::move(a);
    }
    return in;
}

// The next input of execute_many / filter_resample_many: a device tensor as
// long as the first and on its device
void many_in(std::vector<CallIn>& ins, const py::handle& x, Kind k, const std::string& name)
{
    if (!is_device_tensor(x)) throw py::value_error(name + ": device tensors only");
    ins.push_back(in_1d(x, k));
    if (ins.back().n != ins[0].n) throw py::value_error(name + ": every input must have the same length");
    if (!ins.back().device.equal(ins[0].device)) throw py::value_error(name + ": every input must be on the same device");
}

// A [rows, K] input of the class `name`; 1-D stands for one row where `vec`
// says so.  A device tensor whose columns are one sample apart and whose rows
// do not overlap is read in place; any other is refused or copied.
enum class Strided { refuse, copy };
CallIn in_rows(const py::handle& x, Kind k, unsigned rows, const std::string& name, bool vec, Strided policy)
{
    auto check_rows = [&](py::ssize_t ndim, py::ssize_t got) {
        if (ndim != 2)
            throw py::value_error(name + ": the input must be 2-D, [nchan, K]" + (vec ? " (1-D when nchan is 1)" : ""));
        if (got != (py::ssize_t)rows)
            throw py::value_error(name + ": the input has " + std::to_string(got) + " rows, nchan is " +
                                  std::to_string(rows));
    };
    CallIn in;
    if (!is_device_tensor(x)) {
        py::array a = host_in(x, k);
        if (vec && rows == 1 && a.ndim() == 1) a = a.reshape({(py::ssize_t)1, a.shape(0)});
        check_rows(a.ndim(), a.ndim() == 2 ? a.shape(0) : 0);
        in.ptr = a.data();
        in.n = in.ld = (size_t)a.shape(1);
        in.keep = std::move(a);
        return in;
    }
    py::object t = py::reinterpret_borrow<py::object>(x);
    int dim = t.attr("dim")().cast<int>();
    if (vec && rows == 1 && dim == 1) {
        t = t.attr("unsqueeze")(0);
        dim = 2;
    }
    check_rows(dim, dim == 2 ? t.attr("size")(0).cast<py::ssize_t>() : 0);
    t = dev_cast(t, k);
    const size_t K = t.attr("size")(1).cast<size_t>();
    long s0 = t.attr("stride")(0).cast<long>();
    const bool apart = t.attr("stride")(1).cast<long>() != 1, overlap = s0 < (long)K;
    if (policy == Strided::refuse) {
        if (K > 1 && apart)
            throw py::value_error(name + ": the input's columns must be one sample apart (stride(1) == 1)");
        if (rows > 1 && overlap)
            throw py::value_error(name + ": the input's row stride must be at least its number of columns");
        in.ld = rows > 1 ? (size_t)s0 : K;
    } else {
        if (apart || overlap) {
            t = t.attr("contiguous")();
            s0 = t.attr("stride")(0).cast<long>();
        }
        in.ld = std::max<size_t>((size_t)s0, K);
    }
    in.n = K;
    on_device(in, t, DevCheck::full);
    return in;
}

// numpy outputs of host-memory calls: page-locked (ldsp_host_alloc) from 64 KB up, so
// the call DMAs into them and a following call DMAs out of them without a staging
// copy (the README chain hands each stage's array to the next); ordinary
// writeable numpy arrays otherwise alike.  Pageable when the pool is exhausted.
using Shape = std::vector<py::ssize_t>;
py::array host_array(Kind k, size_t n)
{
    const size_t bytes = n * kind_size(k);
    void* p = nullptr;
    if (bytes >= ((size_t)64 << 10) && ldsp_host_alloc(bytes, &p) == LDSP_OK) {
        py::capsule owner(p, [](void* q) { ldsp_host_free(q); });
        return py::array(np_dtype(k), Shape{(py::ssize_t)n}, Shape{(py::ssize_t)kind_size(k)}, p, owner);
    }
    return py::array(np_dtype(k), Shape{(py::ssize_t)n});
}

// A call's result where its input is: a device tensor on the input's device or
// a numpy array (1-D: host_array; 2-D: an ordinary array), n or [n, cols] of kind k.
struct CallOut {
    py::object obj;
    void* ptr = nullptr;
};
CallOut make_out(const CallIn& in, Kind k, size_t n, py::ssize_t cols = -1)
{
    CallOut o;
    if (in.dev) {
        py::object& torch = torch_mod();
        py::dict kw;
        kw["dtype"] = torch.attr(torch_name(k));
        kw["device"] = in.device;
        o.obj = cols < 0 ? torch.attr("empty")(py::int_(n), **kw) : torch.attr("empty")(py::make_tuple(n, cols), **kw);
        o.ptr = tptr(o.obj);
        return o;
    }
    py::array a = cols < 0 ? host_array(k, n) : py::array(np_dtype(k), Shape{(py::ssize_t)n, cols});
    o.ptr = a.mutable_data();
    o.obj = std::move(a);
    return o;
}

// f(mem, stream) -> rc where the input is: on the device on its stream, the GIL
// held; on the host with the GIL released while the call waits for the GPU.
template <typename F>
void invoke(const CallIn& in, F&& f)
{
    int rc;
    if (in.dev) {
        rc = f(LDSP_MEM_DEVICE, in.stream);
    } else {
        py::gil_scoped_release rel;
        rc = f(LDSP_MEM_HOST, (void*)nullptr);
    }
    check(rc);
}

// Same-length stage (FIR / IIR / NCO / AGC): in -> out of the given kinds
template <typename F>
py::object run_same(const py::handle& x, Kind kin, Kind kout, F&& exec)
{
    const CallIn in = in_1d(x, kin);
    CallOut out = make_out(in, kout, in.n);
    invoke(in, [&](int mem, void* s) { return exec(in.ptr, in.n, out.ptr, mem, s); });
    return out.obj;
}

// 1-D in, num_outputs(n) out (the resamplers, FMStereo, filter_resample)
template <typename N, typename F>
py::object run_counted(const py::handle& x, Kind kin, Kind kout, N&& num_outputs, F&& exec)
{
    const CallIn in = in_1d(x, kin);
    size_t nout = 0, nw = 0;
    check(num_outputs(in.n, &nout));
    CallOut out = make_out(in, kout, nout);
    invoke(in, [&](int mem, void* s) { return exec(in.ptr, in.n, out.ptr, nout, &nw, mem, s); });
    return out.obj;
}

// 1-D in (complex64, or int16 IQ pairs converted by the kernel's loads: exec16),
// complex64[rows, num_outputs(n)] out (Channelizer, Downconverter)
template <typename Q, typename E>
py::object run_to_rows(Q q, const py::handle& x, bool iq16, unsigned rows, int (*num_outputs)(Q, size_t, size_t*),
                       E exec, E exec16)
{
    const CallIn in = in_1d(x, iq16 ? Kind::i16 : Kind::c64);
    size_t K = 0, nw = 0;
    check(num_outputs(q, in.n, &K));
    CallOut out = make_out(in, Kind::c64, rows, (py::ssize_t)K);
    invoke(in, [&](int mem, void* s) { return (iq16 ? exec16 : exec)(q, in.ptr, in.n, out.ptr, K, &nw, mem, s); });
    return out.obj;
}

// A row image in (in_rows), num_outputs(K) per row out: kout[orows, N], or
// kout[N] where orows < 0 (FMBank, AudioBank, Synthesizer)
template <typename Q>
py::object run_from_rows(Q q, const CallIn& in, Kind kout, py::ssize_t orows, int (*num_outputs)(Q, size_t, size_t*),
                         int (*exec)(Q, const void*, size_t, size_t, void*, size_t, size_t*, int, void*))
{
    size_t N = 0, nw = 0;
    check(num_outputs(q, in.n, &N));
    CallOut out = orows < 0 ? make_out(in, kout, N) : make_out(in, kout, (size_t)orows, (py::ssize_t)N);
    invoke(in, [&](int mem, void* s) { return exec(q, in.ptr, in.ld, in.n, out.ptr, N, &nw, mem, s); });
    return out.obj;
}

// The optional Fc of the banks: None stands for the C ABI's default (0)
float opt_cutoff(const py::object& fc, const std::string& name)
{
    if (fc.is_none()) return 0.0f;
    const float f = fc.cast<float>();
    if (!(f > 0.0f && f < 0.5f)) throw py::value_error(name + ": Fc must lie in (0, 0.5)");
    return f;
}

// k / N wrapped into [-0.5, 0.5)
py::array_t<double> wrapped_centers(unsigned N)
{
    py::array_t<double> c(N);
    for (unsigned k = 0; k < N; k++) c.mutable_at(k) = std::fmod((double)k / N + 0.5, 1.0) - 0.5;
    return c;
}

std::vector<float> to_fvec(const py::handle& h)
{
    farr a = farr::ensure(h);
    if (!a) throw py::error_already_set();
    return std::vector<float>(a.data(), a.data() + a.size());
}

// ------------------------------------------------------------------ FIR
struct FIR {
    Handle<ldsp_firfilt_t, ldsp_firfilt_destroy> q;
    bool cplx = false;
    cf freqresponse(float f)
    {
        float re, im;
        check(ldsp_firfilt_freqresponse(q, f, &re, &im));
        return cf(re, im);
    }
    py::object call(const py::handle& x)
    {
        return run_same(x, kind_of(cplx), kind_of(cplx), [&](const void* xi, size_t n, void* yo, int mem, void* s) {
            return ldsp_firfilt_execute(q, xi, n, yo, mem, s);
        });
    }
    void reset() { check(ldsp_firfilt_reset(q)); }
    bool get_exact() { return exact_; }
    void set_exact(bool e)
    {
        check(ldsp_firfilt_set_mode(q, e ? LDSP_MODE_EXACT : LDSP_MODE_FAST));
        exact_ = e;
    }
    // "fast" (default: overlap-save FFT for complex data and 48..1025 taps),
    // "direct" (register-blocked direct form), "exact" (liquid order, bitwise)
    std::string get_mode()
    {
        int m;
        check(ldsp_firfilt_get_mode(q, &m));
        return m == LDSP_MODE_EXACT ? "exact" : (m == LDSP_MODE_DIRECT ? "direct" : "fast");
    }
    void set_mode(const std::string& m)
    {
        int v;
        if (m == "fast") v = LDSP_MODE_FAST;
        else if (m == "direct") v = LDSP_MODE_DIRECT;
        else if (m == "exact") v = LDSP_MODE_EXACT;
        else throw py::value_error("mode must be 'fast', 'direct' or 'exact'");
        check(ldsp_firfilt_set_mode(q, v));
        exact_ = v == LDSP_MODE_EXACT;
    }
    py::array_t<float> taps()
    {
        unsigned n;
        check(ldsp_firfilt_get_length(q, &n));
        py::array_t<float> h(n);
        check(ldsp_firfilt_get_taps(q, h.mutable_data()));
        return h;
    }
    float get_scale() { return get_value<float>(ldsp_firfilt_get_scale, q); }
    bool exact_ = false;
};

// RealFIRFilter (firfilter.hpp:5-36)
struct RealFIRFilter : FIR {
    RealFIRFilter() = default;
    explicit RealFIRFilter(const py::handle& h)
    {
        std::vector<float> v = to_fvec(h);
        check(ldsp_firfilt_create(v.data(), (unsigned)v.size(), 0, q.out()));
    }
};
// ComplexFIRFilter: new class (firfilt_crcf semantics of demod.hpp:105,135-136)
struct ComplexFIRFilter : FIR {
    explicit ComplexFIRFilter(const py::handle& h)
    {
        cplx = true;
        std::vector<float> v = to_fvec(h);
        check(ldsp_firfilt_create(v.data(), (unsigned)v.size(), 1, q.out()));
    }
};
// RealDCBlocker (firfilter.hpp:38-50)
struct RealDCBlocker : FIR {
    RealDCBlocker(int m, float as)
    {
        if (m < 1) throw py::value_error("RealDCBlocker: slen must be >= 1");
        check(ldsp_firfilt_create_dc_blocker((unsigned)m, as, 0, q.out()));
    }
};
// RealKaiserBessel (firfilter.hpp:52-66): unit DC gain via set_scale(1/|H(0)|)
struct RealKaiserBessel : FIR {
    RealKaiserBessel(int flen, float fc, float as, float offset)
    {
        if (flen < 1) throw py::value_error("RealKaiserBessel: flen must be >= 1");
        check(ldsp_firfilt_create_kaiser((unsigned)flen, fc, as, offset, 0, q.out()));
        const cf res0 = freqresponse(0.0f);
        check(ldsp_firfilt_set_scale(q, (float)(1.0 / (double)std::abs(res0))));
    }
};

// ------------------------------------------------------------------ resamplers
struct Resampler {
    Handle<ldsp_resamp_t, ldsp_resamp_destroy> q;
    bool cplx;
    float rate_, fc_, as_;
    int m_, npfb_;
    Resampler(float r, int d, float fc, float sbsp, int nf, bool c) : cplx(c), rate_(r), fc_(fc), as_(sbsp), m_(d), npfb_(nf)
    {
        if (d < 1) throw py::value_error("resampler: len must be >= 1");
        if (nf < 1) throw py::value_error("resampler: nfilter must be >= 1");
        check(ldsp_resamp_create(r, (unsigned)d, fc, sbsp, (unsigned)nf, c ? 1 : 0, q.out()));
    }
    // resamp_*_create_default(rate) (RResampler / CResampler, resampler.hpp:10-13,46-49); kind 0 rrrf, 2 crcf
    Resampler(float r, int kind) : cplx(kind != 0), rate_(r), fc_(0.25f), as_(60.0f), m_(7), npfb_(256)
    {
        check(ldsp_resamp_create_default(r, kind, q.out()));
    }
    void reset() { check(ldsp_resamp_reset(q)); }
    float get_rate() { return rate_; }
    void set_rate(float r)
    {
        check(ldsp_resamp_set_rate(q, r));
        rate_ = r;
    }
    void print()
    {
        unsigned npfb, sub;
        uint32_t step, phase;
        check(ldsp_resamp_get_info(q, &npfb, &step, &phase, &sub));
        py::print(py::str("<liquid.resamp_{}, rate={}, m={}, as={:.3f}, fc={:.3f}, npfb={}>")
                      .format(cplx ? "cccf" : "rrrf", rate_, m_, as_, fc_, npfb));
    }
    py::object call(const py::handle& x) { return run(x, nullptr); }
    // self(x); with a filter, self(iir(x)) in one pass (filter_resample)
    py::object run(const py::handle& x, ldsp_iirfilt_t iir)
    {
        return run_counted(
            x, kind_of(cplx), kind_of(cplx), [&](size_t n, size_t* k) { return ldsp_resamp_num_outputs(q, n, k); },
            [&](const void* xi, size_t n, void* yo, size_t cap, size_t* nw, int mem, void* s) {
                return iir ? ldsp_iirfilt_resamp_execute(iir, q, xi, n, yo, cap, nw, mem, s)
                           : ldsp_resamp_execute(q, xi, n, yo, cap, nw, mem, s);
            });
    }
};

// ------------------------------------------------------------------ IIR
// filter_type_map / band_type_map (iirfilter.hpp:5-20)
const std::map<std::string, int> kFilterTypes = {{"butter", 0}, {"cheby1", 1}, {"cheby2", 2}, {"ellip", 3}, {"bessel", 4}};
const std::map<std::string, int> kBandTypes = {{"lowpass", 0}, {"highpass", 1}, {"bandpass", 2}, {"bandstop", 3}};

int ftype_of(const std::string& s)
{
    auto it = kFilterTypes.find(s);
    return it == kFilterTypes.end() ? 0 : it->second;
}

struct IIR {
    Handle<ldsp_iirfilt_t, ldsp_iirfilt_destroy> q;
    bool cplx = true;
    bool exact_ = false;
    void reset() { check(ldsp_iirfilt_reset(q)); }
    cf freqresponse(float f)
    {
        float re, im;
        check(ldsp_iirfilt_freqresponse(q, f, &re, &im));
        return cf(re, im);
    }
    py::object call(const py::handle& x)
    {
        return run_same(x, kind_of(cplx), kind_of(cplx), [&](const void* xi, size_t n, void* yo, int mem, void* s) {
            return ldsp_iirfilt_execute(q, xi, n, yo, mem, s);
        });
    }
    // self(bytes_to_iq(raw)) with the conversion fused into the filter's loads
    // (ldsp_iirfilt_execute_iq16): raw is bytes-like / an int16 or uint8 numpy
    // array (host; returns numpy complex64) or an int16 / uint8 device tensor
    // (returns a complex64 device tensor), interleaved int16 (I, Q) pairs.
    py::object from_bytes(const py::handle& b)
    {
        if (!cplx) throw py::value_error("from_bytes: int16 IQ input needs a complex filter");
        return run_same(b, Kind::i16, Kind::c64, [&](const void* xi, size_t n, void* yo, int mem, void* s) {
            return ldsp_iirfilt_execute_iq16(q, xi, n, yo, mem, s);
        });
    }
    bool get_exact() { return exact_; }
    void set_exact(bool e)
    {
        check(ldsp_iirfilt_set_mode(q, e ? LDSP_MODE_EXACT : LDSP_MODE_FAST));
        exact_ = e;
    }
    py::tuple sos()
    {
        unsigned n;
        check(ldsp_iirfilt_get_nsos(q, &n));
        py::array_t<float> B({(py::ssize_t)n, (py::ssize_t)3}), A({(py::ssize_t)n, (py::ssize_t)3});
        check(ldsp_iirfilt_get_sos(q, B.mutable_data(), A.mutable_data()));
        return py::make_tuple(B, A);
    }
    void print()
    {
        unsigned n = 0;
        check(ldsp_iirfilt_get_nsos(q, &n));
        if (n == 0) {
            py::print(py::str("<liquid.iirfilt_{}, type=tf>").format(cplx ? "crcf" : "rrrf"));
            return;
        }
        std::vector<float> B(3 * n), A(3 * n);
        check(ldsp_iirfilt_get_sos(q, B.data(), A.data()));
        py::print(py::str("<liquid.iirfilt_{}, type=sos, order={}>").format(cplx ? "crcf" : "rrrf", 2 * n));
        for (unsigned s = 0; s < n; s++)
            py::print(py::str("  B[{}] = [{:12.8f} {:12.8f} {:12.8f}]  A[{}] = [{:12.8f} {:12.8f} {:12.8f}]")
                          .format(s, B[3 * s], B[3 * s + 1], B[3 * s + 2], s, A[3 * s], A[3 * s + 1], A[3 * s + 2]));
    }
};

// CIIRFilter / RIIRFilter(Bc, Ac) (iirfilter.hpp:23-59, 133-169): transfer function form
struct TFIIR : IIR {
    TFIIR(const py::handle& bc, const py::handle& ac, bool c)
    {
        cplx = c;
        std::vector<float> b = to_fvec(bc), a = to_fvec(ac);
        check(ldsp_iirfilt_create_tf(b.data(), (unsigned)b.size(), a.data(), (unsigned)a.size(), c ? 1 : 0, q.out()));
    }
};

// C/R{Lowpass,Highpass,Bandpass,Bandstop}IIR (iirfilter.hpp:61-131, 171-241)
struct BandIIR : IIR {
    BandIIR(const std::string& typ, int order, float fc, float f0, float ap, float as, int btype, bool c)
    {
        cplx = c;
        if (order < 1) throw py::value_error("iirfilt: order must be >= 1");
        check(ldsp_iirfilt_create_prototype(ftype_of(typ), btype, (unsigned)order, fc, f0, ap, as, c ? 1 : 0, q.out()));
    }
};

// ComplexIIRFilter / RealIIRFilter (iirfilter.hpp:243-356)
struct ProtoIIR : IIR {
    std::string mFt, mBt;
    int mOrder;
    float mFc, mF0, mAp, mAs;
    ProtoIIR(const std::string& ft, const std::string& bt, int order, float fc, float f0, float ap, float as, bool c)
        : mOrder(order), mFc(fc), mF0(f0), mAp(ap), mAs(as)
    {
        cplx = c;
        int fti = 0, bti = 0;
        auto fi = kFilterTypes.find(ft);
        if (fi != kFilterTypes.end()) {
            mFt = ft;
            fti = fi->second;
        }
        auto bi = kBandTypes.find(bt);
        if (bi != kBandTypes.end()) {
            mBt = bt;
            bti = bi->second;
        }
        if (order < 1) throw py::value_error("iirfilt: order must be >= 1");
        check(ldsp_iirfilt_create_prototype(fti, bti, (unsigned)order, fc, f0, ap, as, c ? 1 : 0, q.out()));
    }
};

// DeemphasisFilter (iirfilter.hpp:358-392): 75 us one-pole, b = [1-x], a = [1, -x]
struct DeemphasisFilter : IIR {
    explicit DeemphasisFilter(float sr)
    {
        cplx = false;
        const float x = (float)exp(-1.0 / (75.0E-6 * (double)sr));
        float mA[2], mB[1];
        mA[0] = 1.0f;
        mA[1] = -x;
        mB[0] = (float)(1.0 - (double)x);
        check(ldsp_iirfilt_create_tf(mB, 1, mA, 2, 0, q.out()));
    }
};

// ------------------------------------------------------------------ NCO (nco.hpp:4-81)
struct NCO {
    Handle<ldsp_nco_t, ldsp_nco_destroy> q;
    std::string mType;
    explicit NCO(const std::string& type)
    {
        mType = (type == "nco") ? "nco" : "vco";
        check(ldsp_nco_create(type == "nco" ? 0 : 1, q.out()));
    }
    float frequency() { return get_value<float>(ldsp_nco_get_frequency, q); }
    void set_frequency(float f) { check(ldsp_nco_set_frequency(q, f)); }
    void adjust_frequency(float df) { check(ldsp_nco_adjust_frequency(q, df)); }
    float phase() { return get_value<float>(ldsp_nco_get_phase, q); }
    void set_phase(float p) { check(ldsp_nco_set_phase(q, p)); }
    void adjust_phase(float dp) { check(ldsp_nco_adjust_phase(q, dp)); }
    void set_pll_bandwidth(float bw) { check(ldsp_nco_pll_set_bandwidth(q, bw)); }
    void pll_step(float dph) { check(ldsp_nco_pll_step(q, dph)); }
    void print()
    {
        py::print(py::str("<liquid.nco_crcf, type={}, phase={:.6f}, freq={:.6f}>").format(mType, phase(), frequency()));
    }
    py::tuple state()
    {
        uint32_t t, d;
        check(ldsp_nco_get_state(q, &t, &d));
        return py::make_tuple(t, d);
    }
    py::object mix(const py::handle& x, bool down)
    {
        return run_same(x, Kind::c64, Kind::c64, [&](const void* xi, size_t n, void* yo, int mem, void* s) {
            return ldsp_nco_mix(q, xi, n, yo, down ? 1 : 0, mem, s);
        });
    }
};

// ------------------------------------------------------------------ AGC (agc.hpp:4-149)
// AGC::execute keeps `static int state_last` shared by every instance (agc.hpp:110)
int g_state_last = 0;   // LIQUID_AGC_SQUELCH_UNKNOWN

struct AGC {
    Handle<ldsp_agc_t, ldsp_agc_destroy> q;
    bool mSquelch = false, mLock = false;
    py::object mOnRise = py::none();
    AGC() { check(ldsp_agc_create(q.out())); }
    template <typename T, typename G>
    T get(G g) { return get_value<T>(g, q); }
    void set_bandwidth(float bw) { check(ldsp_agc_set_bandwidth(q, bw)); }
    float get_bandwidth() { return get<float>(ldsp_agc_get_bandwidth); }
    bool get_squelch() { return mSquelch; }
    void set_squelch(bool v)
    {
        mSquelch = v;
        check(ldsp_agc_squelch_enable(q, v ? 1 : 0));
    }
    void set_threshold(double t) { check(ldsp_agc_squelch_set_threshold(q, (float)t)); }
    double get_threshold() { return get<float>(ldsp_agc_squelch_get_threshold); }
    float get_level() { return get<float>(ldsp_agc_get_signal_level); }
    void set_level(float l) { check(ldsp_agc_set_signal_level(q, l)); }
    float get_rssi() { return get<float>(ldsp_agc_get_rssi); }
    void set_rssi(float r) { check(ldsp_agc_set_rssi(q, r)); }
    bool get_lock() { return mLock; }
    void set_lock(bool v)
    {
        mLock = v;
        check(ldsp_agc_lock(q, v ? 1 : 0));
    }
    float get_gain() { return get<float>(ldsp_agc_get_gain); }
    void set_gain(float g) { check(ldsp_agc_set_gain(q, g)); }
    float get_scale() { return get<float>(ldsp_agc_get_scale); }
    void set_scale(float s) { check(ldsp_agc_set_scale(q, s)); }
    int status() { return get<int>(ldsp_agc_squelch_get_status); }
    void reset() { check(ldsp_agc_reset(q)); }
    void print()
    {
        py::print(py::str("<liquid.agc_crcf, rssi={:.4f} dB, gain={:.6f}, bw={:.4f}, locked={}, squelch={}>")
                      .format(get_rssi(), get_gain(), get_bandwidth(), mLock ? "yes" : "no",
                              mSquelch ? "enabled" : "disabled"));
    }
    py::object call(const py::handle& x)
    {
        // Per-sample squelch statuses are needed only while squelch is enabled
        // (otherwise every status is LIQUID_AGC_SQUELCH_DISABLED).
        std::vector<uint8_t> st;
        const bool need = mSquelch;
        py::object out = run_same(x, Kind::c64, Kind::c64, [&](const void* xi, size_t n, void* yo, int mem, void* s) {
            if (need) st.resize(n);
            return ldsp_agc_execute(q, xi, n, yo, need ? st.data() : nullptr, mem, s);
        });
        const size_t n = py::len(out);
        if (!need) {
            if (n > 0) g_state_last = 7;
            return out;
        }
        // replay the onRise transitions in order (after the block; documented)
        for (size_t i = 0; i < st.size(); i++) {
            const int state = st[i];
            if (state != g_state_last) {
                g_state_last = state;
                if (state == 2 && !mOnRise.is_none()) mOnRise();
            }
        }
        return out;
    }
};

// ------------------------------------------------------------------ AmpModem (demod.hpp:221-307)
const std::map<std::string, int> kAmpTypes = {{"dsb", 0}, {"usb", 1}, {"lsb", 2}};

struct AmpModem {
    float mModulation;
    std::string mType;
    bool mCarrier;
    Handle<ldsp_ampmodem_t, ldsp_ampmodem_destroy> q;
    AmpModem(float mod, const std::string& type, bool car) : mModulation(mod), mCarrier(car) { make(mod, type, car); }
    // makeFromArgs (demod.hpp:298-306): a known type string is recorded, an
    // unknown one leaves mType unchanged and demodulates DSB.
    void make(float mod, const std::string& type, bool car)
    {
        Handle<ldsp_ampmodem_t, ldsp_ampmodem_destroy> nq;
        int mt = 0;
        auto it = kAmpTypes.find(type);
        if (it != kAmpTypes.end()) mt = it->second;
        check(ldsp_ampmodem_create(mod, mt, car ? 0 : 1, nq.out()));
        if (it != kAmpTypes.end()) mType = type;
        q = std::move(nq);      // the old modem goes with nq
    }
    // The setters rebuild the modem (state reset, demod.hpp:250-276).  The new
    // handle is created first and swapped in only on success, so a setter that
    // fails leaves the object and its settings unchanged instead of without a modem.
    void set_type(const std::string& type)
    {
        if (type == "dsb" || type == "usb" || type == "lsb") make(mModulation, type, mCarrier);
    }
    std::string get_type() { return mType; }
    void set_modulation(float m)
    {
        make(m, mType, mCarrier);
        mModulation = m;
    }
    float get_modulation() { return mModulation; }
    void set_carrier(bool c)
    {
        make(mModulation, mType, c);
        mCarrier = c;
    }
    bool get_carrier() { return mCarrier; }
    void reset() { check(ldsp_ampmodem_reset(q)); }
    void print()
    {
        py::print(py::str("<liquid.ampmodem, type=\"{}\", carrier_suppressed={}, mod_index={:.6f}>")
                      .format(mType.empty() ? "dsb" : mType, mCarrier ? "false" : "true", mModulation));
    }
    py::tuple pll_state()
    {
        uint32_t t, d;
        check(ldsp_ampmodem_get_pll_state(q, &t, &d));
        return py::make_tuple(t, d);
    }
    py::tuple taps()
    {
        py::array_t<float> lp(51), dc(51), hq(50);
        check(ldsp_ampmodem_get_taps(q, lp.mutable_data(), dc.mutable_data(), hq.mutable_data()));
        return py::make_tuple(lp, dc, hq);
    }
    py::tuple walk_stats()
    {
        uint64_t e, r, f;
        check(ldsp_ampmodem_walk_stats(q, &e, &r, &f));
        return py::make_tuple(e, r, f);
    }
    py::tuple walk_clocks()
    {
        uint64_t w, t;
        check(ldsp_ampmodem_walk_clocks(q, &w, &t));
        return py::make_tuple(w, t);
    }
    py::tuple walk_active()
    {
        uint64_t t, c;
        check(ldsp_ampmodem_walk_active(q, &t, &c));
        return py::make_tuple(t, c);
    }
    py::tuple seq_stats()
    {
        uint64_t b, r;
        check(ldsp_ampmodem_seq_stats(q, &b, &r));
        return py::make_tuple(b, r);
    }
    py::object demod(const py::handle& x)
    {
        return run_same(x, Kind::c64, Kind::f32, [&](const void* xi, size_t n, void* yo, int mem, void* s) {
            return ldsp_ampmodem_demodulate(q, xi, n, yo, mem, s);
        });
    }
};


// ------------------------------------------------------------------ BroadcastAM (demod.hpp:93-153)
struct BroadcastAM {
    Handle<ldsp_bcastam_t, ldsp_bcastam_destroy> q;
    explicit BroadcastAM(int m)
    {
        if (m < 1) throw py::value_error("BroadcastAM: slen must be >= 1");
        check(ldsp_bcastam_create((unsigned)m, q.out()));
    }
    void reset() { check(ldsp_bcastam_reset(q)); }
    bool get_exact() { return get_value<int>(ldsp_bcastam_get_mode, q) == LDSP_MODE_EXACT; }
    void set_exact(bool e) { check(ldsp_bcastam_set_mode(q, e ? LDSP_MODE_EXACT : LDSP_MODE_FAST)); }
    py::object call(const py::handle& x)
    {
        return run_same(x, Kind::c64, Kind::f32, [&](const void* xi, size_t n, void* yo, int mem, void* s) {
            return ldsp_bcastam_demodulate(q, xi, n, yo, nullptr, mem, s);
        });
    }
};

// ------------------------------------------------------------------ FreqDem (demod.hpp:189-219)
struct FreqDem {
    Handle<ldsp_freqdem_t, ldsp_freqdem_destroy> q;
    float kf;
    explicit FreqDem(float k) : kf(k) { check(ldsp_freqdem_create(k, q.out())); }
    void reset() { check(ldsp_freqdem_reset(q)); }
    void print() { py::print(py::str("freqdem:\n    mod. factor :  {:8.4f}").format(kf)); }
    py::object call(const py::handle& x)
    {
        return run_same(x, Kind::c64, Kind::f32, [&](const void* xi, size_t n, void* yo, int mem, void* s) {
            return ldsp_freqdem_demodulate(q, xi, n, yo, mem, s);
        });
    }
};

// ------------------------------------------------------------------ FMStereo (demod.hpp:4-85)
struct FMStereo {
    Handle<ldsp_fmstereo_t, ldsp_fmstereo_destroy> q;
    FMStereo(float iq_rate, float pcm_rate) { check(ldsp_fmstereo_create(iq_rate, pcm_rate, q.out())); }
    void reset() { check(ldsp_fmstereo_reset(q)); }
    py::tuple state()
    {
        uint32_t t, d;
        float pe;
        check(ldsp_fmstereo_get_state(q, &t, &d, &pe));
        return py::make_tuple(t, d, pe);
    }
    // complex64 IQ -> interleaved (L, R) float32
    py::object call(const py::handle& x)
    {
        return run_counted(
            x, Kind::c64, Kind::f32, [&](size_t n, size_t* k) { return ldsp_fmstereo_num_outputs(q, n, k); },
            [&](const void* xi, size_t n, void* yo, size_t cap, size_t* nw, int mem, void* s) {
                return ldsp_fmstereo_execute(q, xi, n, yo, cap, nw, mem, s);
            });
    }
};

// ------------------------------------------------------------------ Delay (utility.hpp:5-57)
struct Delay {
    Handle<ldsp_delay_t, ldsp_delay_destroy> q;
    explicit Delay(int nd)
    {
        if (nd < 0) throw py::value_error("Delay: nd must be >= 0");
        check(ldsp_delay_create((unsigned)nd, q.out()));
    }
    int get_delay() { return (int)get_value<unsigned>(ldsp_delay_get_delay, q); }
    void set_delay(int nd)
    {
        if (nd < 0) throw py::value_error("Delay: nd must be >= 0");
        check(ldsp_delay_set_delay(q, (unsigned)nd));
    }
    // dispatch on dtype like the reference: complex64 / float32, anything else -> None
    py::object call(const py::handle& x)
    {
        Kind k;
        if (!kind_from_dtype(x, &k)) return py::none();
        return run_same(x, k, k, [&](const void* xi, size_t n, void* yo, int mem, void* s) {
            return ldsp_delay_execute(q, xi, n, k == Kind::c64 ? 1 : 0, yo, mem, s);
        });
    }
};

// ------------------------------------------------------------------ firhilbf (demod.hpp:155-187, utility.hpp:71-108)
struct Hilb {
    Handle<ldsp_firhilb_t, ldsp_firhilb_destroy> q;
    Hilb(int m, float as, int op)
    {
        if (m < 0) throw py::value_error("firhilb: m must be >= 2");
        check(ldsp_firhilb_create((unsigned)m, as, op, q.out()));
    }
    // One call: n input samples -> nout(n) outputs per returned array; two arrays
    // (lower, upper) when `both`, else the output goes to y0 (y1 when `second`).
    py::object run(const py::handle& x, Kind kin, Kind kout, size_t (*nout)(size_t), bool both = false,
                   bool second = false)
    {
        const CallIn in = in_1d(x, kin);
        CallOut o0 = make_out(in, kout, nout(in.n)), o1;
        if (both) o1 = make_out(in, kout, nout(in.n));
        void* y0 = both || !second ? o0.ptr : nullptr;
        void* y1 = both ? o1.ptr : (second ? o0.ptr : nullptr);
        invoke(in, [&](int mem, void* s) { return ldsp_firhilb_execute(q, in.ptr, in.n, y0, y1, mem, s); });
        return both ? py::object(py::make_tuple(o0.obj, o1.obj)) : o0.obj;
    }
    static size_t same(size_t n) { return n; }
    static size_t half(size_t n) { return n / 2; }
    static size_t twice(size_t n) { return 2 * n; }
};

// ------------------------------------------------------------------ Channelizer (no reference counterpart)
// Polyphase analysis bank (ldsp.h): complex64[N] -> complex64[nchan, ncols],
// row k the channel centred at k / nchan.  The rows of a device result are
// contiguous views, usable as the channel inputs of execute_many /
// filter_resample_many.
struct Channelizer {
    Handle<ldsp_chan_t, ldsp_chan_destroy> q;
    unsigned M = 0, D = 0, L = 0;
    Channelizer(int nchan, const py::object& decim, int m, const py::object& fc, float as, const py::object& taps)
    {
        if (nchan < 0) throw py::value_error("Channelizer: nchan must be a power of two, at least 4");
        const int d = decim.is_none() ? nchan / 2 : decim.cast<int>();
        if (d < 0) throw py::value_error("Channelizer: decim must be nchan or nchan // 2");
        if (!taps.is_none()) {
            std::vector<float> h = to_fvec(taps);
            check(ldsp_chan_create_taps((unsigned)nchan, (unsigned)d, h.data(), (unsigned)h.size(), q.out()));
        } else {
            if (m < 0) throw py::value_error("Channelizer: m must be >= 1");
            const float f = opt_cutoff(fc, "Channelizer");    // the C ABI's default: 0.5 / nchan
            check(ldsp_chan_create((unsigned)nchan, (unsigned)d, (unsigned)m, f, as, q.out()));
        }
        check(ldsp_chan_get_info(q, &M, &D, &L, nullptr));
    }
    void reset() { check(ldsp_chan_reset(q)); }
    py::array_t<float> taps()
    {
        py::array_t<float> h(L);
        check(ldsp_chan_get_taps(q, h.mutable_data()));
        return h;
    }
    float get_scale() { return get_value<float>(ldsp_chan_get_scale, q); }
    void set_scale(float s) { check(ldsp_chan_set_scale(q, s)); }
    unsigned skip()
    {
        unsigned s;
        check(ldsp_chan_get_info(q, nullptr, nullptr, nullptr, &s));
        return s;
    }
    size_t tile()
    {
        size_t f = 0;
        check(ldsp_debug_chan_tile(M, D, &f));
        return f;
    }
    py::array_t<double> centers() { return wrapped_centers(M); }
    size_t num_outputs(size_t n)
    {
        size_t c = 0;
        check(ldsp_chan_num_outputs(q, n, &c));
        return c;
    }
    py::object run(const py::handle& x, bool iq16)
    {
        return run_to_rows(q.get(), x, iq16, M, ldsp_chan_num_outputs, ldsp_chan_execute, ldsp_chan_execute_iq16);
    }
    py::object call(const py::handle& x) { return run(x, false); }
    // self(bytes_to_iq(raw)) without the complex64 copy: raw as ComplexIIRFilter.from_bytes takes it
    py::object from_bytes(const py::handle& b) { return run(b, true); }
};

// ------------------------------------------------------------------ Downconverter (liquid: nco_crcf + firdecim_crcf)
// Tuned decimating bank (ldsp.h): complex64[N] -> complex64[ntuners, ncols],
// row c the stream mixed down by freqs[c], low-passed and decimated.  The rows
// of a device result are contiguous views, as the Channelizer's.
struct Downconverter {
    Handle<ldsp_ddc_t, ldsp_ddc_destroy> q;
    unsigned D = 0, L = 0;
    static std::vector<double> to_freqs(const py::object& f)
    {
        if (!py::hasattr(f, "__len__")) return {f.cast<double>()};       // a scalar: one tuner
        return f.cast<std::vector<double>>();
    }
    Downconverter(const py::object& freqs, int decim, int m, const py::object& fc, float as, const py::object& taps)
    {
        if (decim < 0) throw py::value_error("Downconverter: decim must be at least 2");
        const std::vector<double> f = to_freqs(freqs);
        if (!taps.is_none()) {
            std::vector<float> h = to_fvec(taps);
            check(ldsp_ddc_create_taps(f.data(), (unsigned)f.size(), (unsigned)decim, h.data(), (unsigned)h.size(), q.out()));
        } else {
            if (m < 0) throw py::value_error("Downconverter: m must be >= 1");
            const float c = opt_cutoff(fc, "Downconverter");  // the C ABI's default: 0.5 / decim
            check(ldsp_ddc_create(f.data(), (unsigned)f.size(), (unsigned)decim, (unsigned)m, c, as, q.out()));
        }
        check(ldsp_ddc_get_info(q, nullptr, &D, &L, nullptr));
    }
    void reset() { check(ldsp_ddc_reset(q)); }
    unsigned ntuners()
    {
        unsigned c;
        check(ldsp_ddc_get_info(q, &c, nullptr, nullptr, nullptr));
        return c;
    }
    py::array_t<uint32_t> words()
    {
        py::array_t<uint32_t> w(ntuners());
        check(ldsp_ddc_get_words(q, w.mutable_data()));
        return w;
    }
    py::array_t<double> get_freqs()
    {
        py::array_t<uint32_t> w = words();
        py::array_t<double> f(w.size());
        for (py::ssize_t c = 0; c < w.size(); c++) f.mutable_at(c) = (double)(int32_t)w.at(c) / 4294967296.0;
        return f;
    }
    void set_freqs(const py::object& freqs)
    {
        const std::vector<double> f = to_freqs(freqs);
        check(ldsp_ddc_set_frequencies(q, f.data(), (unsigned)f.size()));
    }
    py::array_t<float> taps()
    {
        py::array_t<float> h(L);
        check(ldsp_ddc_get_taps(q, h.mutable_data()));
        return h;
    }
    float get_scale() { return get_value<float>(ldsp_ddc_get_scale, q); }
    void set_scale(float s) { check(ldsp_ddc_set_scale(q, s)); }
    unsigned skip()
    {
        unsigned s;
        check(ldsp_ddc_get_info(q, nullptr, nullptr, nullptr, &s));
        return s;
    }
    size_t tile()
    {
        size_t f = 0;
        check(ldsp_debug_ddc_tile(D, L, &f));
        return f;
    }
    size_t num_outputs(size_t n)
    {
        size_t c = 0;
        check(ldsp_ddc_num_outputs(q, n, &c));
        return c;
    }
    void seek(uint64_t T) { check(ldsp_debug_ddc_seek(q, T)); }
    py::object run(const py::handle& x, bool iq16)
    {
        return run_to_rows(q.get(), x, iq16, ntuners(), ldsp_ddc_num_outputs, ldsp_ddc_execute, ldsp_ddc_execute_iq16);
    }
    py::object call(const py::handle& x) { return run(x, false); }
    // self(bytes_to_iq(raw)) without the complex64 copy: raw as ComplexIIRFilter.from_bytes takes it
    py::object from_bytes(const py::handle& b) { return run(b, true); }
};

// ------------------------------------------------------------------ FMBank (liquid: freqdem + firdecim_rrrf per row)
// Discriminator and decimating FIR over bank rows (ldsp.h): complex64[nchan, K]
// -> float32[nchan, ncols].  A device tensor whose columns are one sample apart
// and whose rows do not overlap (a block of rows or a range of columns of a
// Channelizer or Downconverter output) is read in place.
struct FMBank {
    Handle<ldsp_fmbank_t, ldsp_fmbank_destroy> q;
    unsigned C = 0, D = 0, L = 0;
    float kf;
    FMBank(int nchan, float kf_, int decim, int m, const py::object& fc, float as, const py::object& taps) : kf(kf_)
    {
        if (nchan < 0) throw py::value_error("FMBank: nchan must lie in 1 .. 256");
        if (decim < 0) throw py::value_error("FMBank: decim must lie in 1 .. 64");
        if (!taps.is_none()) {
            std::vector<float> h = to_fvec(taps);
            check(ldsp_fmbank_create_taps((unsigned)nchan, kf, (unsigned)decim, h.data(), (unsigned)h.size(), q.out()));
        } else {
            if (m < 0) throw py::value_error("FMBank: m must be >= 1");
            const float c = opt_cutoff(fc, "FMBank");         // the C ABI's default: 0.5 / decim
            check(ldsp_fmbank_create((unsigned)nchan, kf, (unsigned)decim, (unsigned)m, c, as, q.out()));
        }
        check(ldsp_fmbank_get_info(q, &C, &D, &L, nullptr));
    }
    void reset() { check(ldsp_fmbank_reset(q)); }
    py::array_t<float> taps()
    {
        py::array_t<float> h(L);
        if (L) check(ldsp_fmbank_get_taps(q, h.mutable_data()));
        return h;
    }
    float get_scale() { return get_value<float>(ldsp_fmbank_get_scale, q); }
    void set_scale(float s) { check(ldsp_fmbank_set_scale(q, s)); }
    unsigned skip()
    {
        unsigned s;
        check(ldsp_fmbank_get_info(q, nullptr, nullptr, nullptr, &s));
        return s;
    }
    size_t tile()
    {
        size_t f = 0;
        check(ldsp_debug_fmbank_tile(D, L, &f));
        return f;
    }
    size_t num_outputs(size_t K)
    {
        size_t c = 0;
        check(ldsp_fmbank_num_outputs(q, K, &c));
        return c;
    }
    py::object call(const py::handle& x)
    {
        return run_from_rows(q.get(), in_rows(x, Kind::c64, C, "FMBank", true, Strided::refuse), Kind::f32, C,
                             ldsp_fmbank_num_outputs, ldsp_fmbank_execute);
    }
};

// ------------------------------------------------------------------ SquelchBank (liquid: the squelch half of agc_crcf per row, per block)
// Input as the FMBank's.  Each call returns new arrays where its input is;
// status and level keep the last call's.
struct SquelchBank {
    Handle<ldsp_sqbank_t, ldsp_sqbank_destroy> q;
    unsigned C = 0, B = 0, tmo = 0;
    double alpha = 0.0;
    py::object last_status = py::none(), last_level = py::none();
    static std::vector<double> to_dvec(const py::object& o)
    {
        auto a = py::array_t<double, py::array::c_style | py::array::forcecast>::ensure(o);
        if (!a) throw py::error_already_set();
        return std::vector<double>(a.data(), a.data() + a.size());
    }
    SquelchBank(int nchan, int block, const py::object& threshold, double bandwidth, int timeout)
    {
        if (nchan < 0) throw py::value_error("SquelchBank: nchan must lie in 1 .. 256");
        if (block < 0) throw py::value_error("SquelchBank: block must lie in 16 .. 4096");
        if (timeout < 0) throw py::value_error("SquelchBank: timeout must be >= 1");
        const std::vector<double> t = to_dvec(threshold);
        if (t.empty()) throw py::value_error("SquelchBank: one threshold or one per row");
        check(ldsp_sqbank_create((unsigned)nchan, (unsigned)block, bandwidth, t[0], (unsigned)timeout, q.out()));
        check(ldsp_sqbank_get_info(q, &C, &B, &alpha, &tmo, nullptr));
        if (t.size() > 1) check(ldsp_sqbank_set_thresholds(q, t.data(), (unsigned)t.size()));
    }
    void reset() { check(ldsp_sqbank_reset(q)); }
    py::array_t<double> get_threshold()
    {
        py::array_t<double> t(C);
        check(ldsp_sqbank_get_thresholds(q, t.mutable_data(), nullptr));
        return t;
    }
    void set_threshold(const py::object& o)
    {
        const std::vector<double> t = to_dvec(o);
        check(ldsp_sqbank_set_thresholds(q, t.data(), (unsigned)t.size()));
    }
    py::array_t<float> threshold_linear()
    {
        py::array_t<float> t(C);
        check(ldsp_sqbank_get_thresholds(q, nullptr, t.mutable_data()));
        return t;
    }
    unsigned fill()
    {
        unsigned f;
        check(ldsp_sqbank_get_info(q, nullptr, nullptr, nullptr, nullptr, &f));
        return f;
    }
    size_t tile()
    {
        size_t t;
        check(ldsp_debug_sqbank_tile(B, &t));
        return t;
    }
    size_t num_outputs(size_t K)
    {
        size_t n;
        check(ldsp_sqbank_num_outputs(q, K, &n));
        return n;
    }
    py::tuple state()
    {
        py::array_t<int> mode(C);
        py::array_t<unsigned> timer(C);
        py::array_t<double> s(C);
        check(ldsp_sqbank_get_state(q, mode.mutable_data(), timer.mutable_data(), s.mutable_data()));
        return py::make_tuple(mode, timer, s);
    }
    // status, level and (gate) the gated rows of the call's whole blocks
    py::object run(const py::handle& x, bool gate)
    {
        const CallIn in = in_rows(x, Kind::c64, C, "SquelchBank", true, Strided::refuse);
        size_t N = 0, nw = 0;
        check(ldsp_sqbank_num_outputs(q, in.n, &N));
        CallOut st = make_out(in, Kind::u8, C, (py::ssize_t)N), lv = make_out(in, Kind::f32, C, (py::ssize_t)N), y;
        if (gate) y = make_out(in, Kind::c64, C, (py::ssize_t)(N * B));
        invoke(in, [&](int mem, void* s) {
            return ldsp_sqbank_execute(q, in.ptr, in.ld, in.n, (uint8_t*)st.ptr, N, (float*)lv.ptr, N, y.ptr, N * B, &nw,
                                       mem, s);
        });
        last_status = st.obj;
        last_level = lv.obj;
        return gate ? y.obj : py::object(py::make_tuple(st.obj, lv.obj));
    }
    py::object call(const py::handle& x) { return run(x, true); }
    py::object measure(const py::handle& x) { return run(x, false); }
};

// ------------------------------------------------------------------ AGCBank (no reference counterpart; AGC restates liquid's loop)
// Look-ahead hang AGC over bank rows (ldsp.h): float32[nchan, K] (input as the
// AudioBank's: a bank's output is read in place) or complex64[nchan, K] ->
// the emitted blocks, the same kind.  peak_q, gain_q and gain_db keep the last
// call's tracked blocks.
struct AGCBank {
    Handle<ldsp_agcbank_t, ldsp_agcbank_destroy> q;
    unsigned C = 0, B = 0, H = 0;
    double decay = 0.0, max_gain = 0.0;
    bool cplx = false;
    py::object last_peak = py::none(), last_gain = py::none();
    AGCBank(int nchan, int block, const py::object& target, double max_gain_, int hang, double decay_, bool complex_)
    {
        if (nchan < 0) throw py::value_error("AGCBank: nchan must lie in 1 .. 256");
        if (block < 0) throw py::value_error("AGCBank: block must lie in 16 .. 4096");
        if (hang < 0) throw py::value_error("AGCBank: hang must lie in 0 .. 255");
        const std::vector<double> t = SquelchBank::to_dvec(target);
        if (t.empty()) throw py::value_error("AGCBank: one target or one per row");
        check(ldsp_agcbank_create((unsigned)nchan, (unsigned)block, t.data(), (unsigned)t.size(), max_gain_, (unsigned)hang,
                                  decay_, complex_ ? 1 : 0, q.out()));
        int cx = 0;
        check(ldsp_agcbank_get_info(q, &C, &B, &H, &decay, &max_gain, nullptr, &cx, nullptr));
        cplx = cx != 0;
    }
    void reset() { check(ldsp_agcbank_reset(q)); }
    py::array_t<double> target()
    {
        py::array_t<double> t(C);
        check(ldsp_agcbank_get_info(q, nullptr, nullptr, nullptr, nullptr, nullptr, t.mutable_data(), nullptr, nullptr));
        return t;
    }
    unsigned fill()
    {
        unsigned f;
        check(ldsp_agcbank_get_info(q, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &f));
        return f;
    }
    size_t num_outputs(size_t K)
    {
        size_t ne;
        check(ldsp_agcbank_num_outputs(q, K, nullptr, &ne));
        return ne * B;
    }
    py::tuple state()
    {
        py::array_t<int32_t> level(C), peaks({(py::ssize_t)C, (py::ssize_t)H});
        py::array_t<float> gains({(py::ssize_t)C, (py::ssize_t)2});
        check(ldsp_agcbank_get_state(q, level.mutable_data(), peaks.mutable_data(), gains.mutable_data()));
        return py::make_tuple(level, peaks, gains);
    }
    py::object gain_db()
    {
        if (last_gain.is_none()) return py::none();
        const double c = 20.0 * std::log10(2.0) / 16777216.0;   // dB per unit
        if (is_device_tensor(last_gain)) return last_gain.attr("double")().attr("mul")(c).attr("float")();
        return last_gain.attr("astype")("float64").attr("__mul__")(c).attr("astype")("float32");
    }
    py::object call(const py::handle& x)
    {
        const Kind kd = kind_of(cplx);
        const CallIn in = in_rows(x, kd, C, "AGCBank", true, Strided::refuse);
        size_t nt = 0, ne = 0, nw = 0;
        check(ldsp_agcbank_num_outputs(q, in.n, &nt, &ne));
        CallOut y = make_out(in, kd, C, (py::ssize_t)(ne * B)), pq = make_out(in, Kind::i32, C, (py::ssize_t)nt),
                gq = make_out(in, Kind::i32, C, (py::ssize_t)nt);
        invoke(in, [&](int mem, void* s) {
            return ldsp_agcbank_execute(q, in.ptr, in.ld, in.n, y.ptr, ne * B, (int32_t*)pq.ptr, (int32_t*)gq.ptr, nt, &nw,
                                        mem, s);
        });
        last_peak = pq.obj;
        last_gain = gq.obj;
        return y.obj;
    }
};

// ------------------------------------------------------------------ ToneBank (no reference counterpart)
// Per-row tone detector and tone squelch over bank rows (ldsp.h): float32[nchan, K]
// (input as the AudioBank's: a bank's output is read in place) -> the gated rows
// or (tone, power).  tone, power and open keep the last call's.
struct ToneBank {
    Handle<ldsp_tonebank_t, ldsp_tonebank_destroy> q;
    unsigned C = 0, F = 0, B = 0, hold = 0;
    int window = 0;
    py::object last_tone = py::none(), last_power = py::none(), last_open = py::none();
    static std::vector<int> to_ivec(const py::object& o, const char* what)
    {
        const std::vector<double> d = SquelchBank::to_dvec(o);
        std::vector<int> v(d.size());
        for (size_t i = 0; i < d.size(); i++) {
            if (!(d[i] >= -1.0 && d[i] <= 64.0) || d[i] != std::floor(d[i])) throw py::value_error(what);
            v[i] = (int)d[i];
        }
        return v;
    }
    ToneBank(int nchan, const py::object& tones, int block, const std::string& win, double dominance, float floor_,
             int hold_, const py::object& want)
    {
        if (nchan < 0) throw py::value_error("ToneBank: nchan must lie in 1 .. 256");
        if (block < 0) throw py::value_error("ToneBank: block must be a multiple of 64 in 64 .. 16384");
        if (hold_ < 0) throw py::value_error("ToneBank: hold must lie in 0 .. 64");
        if (win != "hann" && win != "rect") throw py::value_error("ToneBank: window must be 'hann' or 'rect'");
        const std::vector<double> f = SquelchBank::to_dvec(tones);
        check(ldsp_tonebank_create((unsigned)nchan, f.data(), (unsigned)f.size(), (unsigned)block,
                                   win == "hann" ? LDSP_TONE_HANN : LDSP_TONE_RECT, dominance, floor_, (unsigned)hold_,
                                   q.out()));
        check(ldsp_tonebank_get_info(q, &C, &F, &B, &window, &hold, nullptr));
        if (!want.is_none()) set_want(want);
    }
    void reset() { check(ldsp_tonebank_reset(q)); }
    py::array_t<double> tones()
    {
        py::array_t<double> f(F);
        check(ldsp_tonebank_get_tables(q, f.mutable_data(), nullptr, nullptr, nullptr));
        return f;
    }
    py::array_t<float> tables()
    {
        py::array_t<float> t({(py::ssize_t)2, (py::ssize_t)F, (py::ssize_t)B});
        check(ldsp_tonebank_get_tables(q, nullptr, t.mutable_data(), t.mutable_data() + (size_t)F * B, nullptr));
        return t;
    }
    double sumw()
    {
        double s;
        check(ldsp_tonebank_get_tables(q, nullptr, nullptr, nullptr, &s));
        return s;
    }
    py::array_t<int> get_want()
    {
        py::array_t<int> w(C);
        check(ldsp_tonebank_get_want(q, w.mutable_data()));
        return w;
    }
    void set_want(const py::object& o)
    {
        const std::vector<int> w = to_ivec(o, "ToneBank: want must be integers in -1 .. F - 1");
        check(ldsp_tonebank_set_want(q, w.data(), (unsigned)w.size()));
    }
    double get_dominance() { return get_value<double>(ldsp_tonebank_get_dominance, q); }
    void set_dominance(double d) { check(ldsp_tonebank_set_dominance(q, d)); }
    float get_floor() { return get_value<float>(ldsp_tonebank_get_floor, q); }
    void set_floor(float f) { check(ldsp_tonebank_set_floor(q, f)); }
    unsigned fill()
    {
        unsigned f;
        check(ldsp_tonebank_get_info(q, nullptr, nullptr, nullptr, nullptr, nullptr, &f));
        return f;
    }
    size_t tile()
    {
        size_t t;
        check(ldsp_debug_tonebank_tile(B, &t));
        return t;
    }
    size_t num_outputs(size_t K)
    {
        size_t n;
        check(ldsp_tonebank_num_outputs(q, K, &n));
        return n;
    }
    py::array_t<int> state()
    {
        py::array_t<int> s(C);
        check(ldsp_tonebank_get_state(q, s.mutable_data()));
        return s;
    }
    // tone, power, open and (gate) the gated rows of the call's whole blocks
    py::object run(const py::handle& x, bool gate)
    {
        const CallIn in = in_rows(x, Kind::f32, C, "ToneBank", true, Strided::refuse);
        size_t N = 0, nw = 0;
        check(ldsp_tonebank_num_outputs(q, in.n, &N));
        CallOut tn = make_out(in, Kind::i8, C, (py::ssize_t)N), op = make_out(in, Kind::u8, C, (py::ssize_t)N), y;
        CallOut pw = make_out(in, Kind::f32, (size_t)C * N, (py::ssize_t)F);
        if (gate) y = make_out(in, Kind::f32, C, (py::ssize_t)(N * B));
        invoke(in, [&](int mem, void* s) {
            return ldsp_tonebank_execute(q, (const float*)in.ptr, in.ld, in.n, (float*)pw.ptr, N * F, (int8_t*)tn.ptr, N,
                                         (uint8_t*)op.ptr, N, (float*)y.ptr, N * B, &nw, mem, s);
        });
        last_tone = tn.obj;
        last_power = pw.obj.attr("reshape")(py::make_tuple(C, N, F));
        last_open = op.obj;
        return gate ? y.obj : py::object(py::make_tuple(last_tone, last_power));
    }
    py::object call(const py::handle& x) { return run(x, true); }
    py::object measure(const py::handle& x) { return run(x, false); }
};

// ------------------------------------------------------------------ StereoBank (no reference counterpart; FMStereo is another decoder)
// Feed-forward FM stereo decoder over bank rows (ldsp.h): float32[nchan, K] of
// multiplex -> float32[nchan, 2, ncols], left at [:, 0] and right at [:, 1]; its
// [2 nchan, ncols] view is an AudioBank's input.  Input as the AudioBank's: an
// FMBank output, a block of rows or a range of columns of one is read in place.
struct StereoBank {
    Handle<ldsp_stbank_t, ldsp_stbank_destroy> q;
    unsigned C = 0, D = 0, L = 0;
    uint32_t w = 0;
    StereoBank(int nchan, double pilot, int decim, const py::object& ntaps, float as, float thr, const py::object& taps,
               const py::object& ptaps)
    {
        if (nchan < 0) throw py::value_error("StereoBank: nchan must lie in 1 .. 128");
        if (decim < 0) throw py::value_error("StereoBank: decim must lie in 1 .. 32");
        if (taps.is_none() != ptaps.is_none())
            throw py::value_error("StereoBank: taps and pilot_taps come together");
        if (!taps.is_none()) {
            if (!ntaps.is_none()) throw py::value_error("StereoBank: ntaps or taps, not both");
            std::vector<float> h = to_fvec(taps), g = to_fvec(ptaps);
            check(ldsp_stbank_create_taps((unsigned)nchan, pilot, (unsigned)decim, h.data(), (unsigned)h.size(), g.data(),
                                          (unsigned)g.size(), thr, q.out()));
        } else {
            const long n = ntaps.is_none() ? 0 : ntaps.cast<long>();
            if (!ntaps.is_none() && (n < 1 || n > 1025)) throw py::value_error("StereoBank: ntaps must lie in 1 .. 1025");
            check(ldsp_stbank_create((unsigned)nchan, pilot, (unsigned)decim, (unsigned)n, as, thr, q.out()));
        }
        check(ldsp_stbank_get_info(q, &C, &D, &L, nullptr, &w));
    }
    void reset() { check(ldsp_stbank_reset(q)); }
    py::array_t<float> taps()
    {
        py::array_t<float> h(L);
        check(ldsp_stbank_get_taps(q, h.mutable_data(), nullptr));
        return h;
    }
    py::array_t<float> pilot_taps()
    {
        py::array_t<float> g(L);
        check(ldsp_stbank_get_taps(q, nullptr, g.mutable_data()));
        return g;
    }
    float get_threshold() { return get_value<float>(ldsp_stbank_get_threshold, q); }
    void set_threshold(float t) { check(ldsp_stbank_set_threshold(q, t)); }
    unsigned skip()
    {
        unsigned s;
        check(ldsp_stbank_get_info(q, nullptr, nullptr, nullptr, &s, nullptr));
        return s;
    }
    size_t tile()
    {
        size_t f = 0;
        check(ldsp_debug_stbank_tile(D, L, &f));
        return f;
    }
    size_t num_outputs(size_t K)
    {
        size_t c = 0;
        check(ldsp_stbank_num_outputs(q, K, &c));
        return c;
    }
    py::array_t<float> pilot_level()
    {
        py::array_t<float> v(C);
        check(ldsp_stbank_get_pilot_level(q, v.mutable_data()));
        return v;
    }
    py::array_t<bool> stereo()
    {
        const py::array_t<float> v = pilot_level();
        const float t = get_threshold();
        py::array_t<bool> s(C);
        for (unsigned c = 0; c < C; c++) s.mutable_at(c) = v.at(c) > t;
        return s;
    }
    py::object call(const py::handle& x)
    {
        py::object y = run_from_rows(q.get(), in_rows(x, Kind::f32, C, "StereoBank", true, Strided::refuse), Kind::f32,
                                     2 * (py::ssize_t)C, ldsp_stbank_num_outputs, ldsp_stbank_execute);
        return y.attr("reshape")(py::make_tuple(C, 2, y.attr("shape").attr("__getitem__")(1)));
    }
};

// ------------------------------------------------------------------ AMBank (no reference counterpart; AmpModem is another demodulator)
// Feed-forward coherent AM demodulator over bank rows (ldsp.h): complex64[nchan, K]
// -> float32[nchan, ncols], an AudioBank's input.  Input as the FMBank's: a
// Channelizer output, a block of rows or a range of columns of one is read in place.
struct AMBank {
    Handle<ldsp_ambank_t, ldsp_ambank_destroy> q;
    unsigned C = 0, D = 0, L = 0;
    AMBank(int nchan, int decim, const py::object& audio, double carrier, const py::object& ntaps, float as, float thr,
           const py::object& taps, const py::object& ctaps)
    {
        if (nchan < 0) throw py::value_error("AMBank: nchan must lie in 1 .. 256");
        if (decim < 0) throw py::value_error("AMBank: decim must lie in 1 .. 32");
        if (taps.is_none() != ctaps.is_none()) throw py::value_error("AMBank: taps and carrier_taps come together");
        if (!taps.is_none()) {
            if (!ntaps.is_none()) throw py::value_error("AMBank: ntaps or taps, not both");
            std::vector<float> h = to_fvec(taps), g = to_fvec(ctaps);
            check(ldsp_ambank_create_taps((unsigned)nchan, (unsigned)decim, h.data(), (unsigned)h.size(), g.data(),
                                          (unsigned)g.size(), thr, q.out()));
        } else {
            const long n = ntaps.is_none() ? 0 : ntaps.cast<long>();
            if (!ntaps.is_none() && (n < 1 || n > 1025)) throw py::value_error("AMBank: ntaps must lie in 1 .. 1025");
            const double fa = audio.is_none() ? 0.0 : audio.cast<double>();
            if (!audio.is_none() && !(fa > 0.0)) throw py::value_error("AMBank: audio must lie in (carrier, 0.5]");
            check(ldsp_ambank_create((unsigned)nchan, (unsigned)decim, fa, carrier, (unsigned)n, as, thr, q.out()));
        }
        check(ldsp_ambank_get_info(q, &C, &D, &L, nullptr));
    }
    void reset() { check(ldsp_ambank_reset(q)); }
    py::array_t<float> taps()
    {
        py::array_t<float> h(L);
        check(ldsp_ambank_get_taps(q, h.mutable_data(), nullptr, nullptr));
        return h;
    }
    py::array_t<float> carrier_taps()
    {
        py::array_t<float> g(L);
        check(ldsp_ambank_get_taps(q, nullptr, g.mutable_data(), nullptr));
        return g;
    }
    py::array_t<float> band_taps()
    {
        py::array_t<float> d(L);
        check(ldsp_ambank_get_taps(q, nullptr, nullptr, d.mutable_data()));
        return d;
    }
    float get_threshold() { return get_value<float>(ldsp_ambank_get_threshold, q); }
    void set_threshold(float t) { check(ldsp_ambank_set_threshold(q, t)); }
    unsigned skip()
    {
        unsigned s;
        check(ldsp_ambank_get_info(q, nullptr, nullptr, nullptr, &s));
        return s;
    }
    size_t tile()
    {
        size_t f = 0;
        check(ldsp_debug_ambank_tile(D, L, &f));
        return f;
    }
    size_t num_outputs(size_t K)
    {
        size_t c = 0;
        check(ldsp_ambank_num_outputs(q, K, &c));
        return c;
    }
    py::array_t<float> carrier_level()
    {
        py::array_t<float> v(C);
        check(ldsp_ambank_get_carrier_level(q, v.mutable_data()));
        return v;
    }
    py::array_t<bool> carrier_present()
    {
        const py::array_t<float> v = carrier_level();
        const float t = get_threshold();
        py::array_t<bool> s(C);
        for (unsigned c = 0; c < C; c++) s.mutable_at(c) = v.at(c) > t;
        return s;
    }
    py::object call(const py::handle& x)
    {
        return run_from_rows(q.get(), in_rows(x, Kind::c64, C, "AMBank", true, Strided::refuse), Kind::f32, C,
                             ldsp_ambank_num_outputs, ldsp_ambank_execute);
    }
};

// ------------------------------------------------------------------ SSBBank (liquid: ampmodem's SSB modes, one untuned stream per object)
// Tuned single-sideband demodulator over bank rows (ldsp.h): complex64[nchan, K]
// -> float32[nchan, ncols], an AudioBank's input.  Input as the AMBank's: a
// Channelizer output, a block of rows or a range of columns of one is read in place.
struct SSBBank {
    Handle<ldsp_ssbbank_t, ldsp_ssbbank_destroy> q;
    unsigned C = 0, D = 0, L = 0;
    // a scalar or a sequence of n entries
    static std::vector<double> to_bfos(const py::object& o, size_t n)
    {
        if (!py::hasattr(o, "__len__")) return std::vector<double>(n, o.cast<double>());
        std::vector<double> v = o.cast<std::vector<double>>();
        if (v.size() != n) throw py::value_error("SSBBank: bfo takes a scalar or one entry per row");
        return v;
    }
    static int to_side(const py::handle& h)
    {
        if (py::isinstance<py::str>(h)) {
            const std::string s = h.cast<std::string>();
            if (s == "usb") return 1;
            if (s == "lsb") return -1;
        }
        throw py::value_error("SSBBank: a sideband is 'usb' or 'lsb'");
    }
    static std::vector<int> to_sides(const py::object& o, size_t n)
    {
        if (py::isinstance<py::str>(o)) return std::vector<int>(n, to_side(o));
        if (!py::hasattr(o, "__len__")) throw py::value_error("SSBBank: a sideband is 'usb' or 'lsb'");
        std::vector<int> v;
        for (const py::handle& h : o) v.push_back(to_side(h));
        if (v.size() != n) throw py::value_error("SSBBank: sideband takes one name or one per row");
        return v;
    }
    SSBBank(int nchan, int decim, double lo, const py::object& hi, const py::object& bfo, const py::object& sideband,
            const py::object& ntaps, float as, const py::object& taps)
    {
        if (nchan < 1 || nchan > 256) throw py::value_error("SSBBank: nchan must lie in 1 .. 256");
        if (decim < 0) throw py::value_error("SSBBank: decim must lie in 1 .. 32");
        const double fh = hi.is_none() ? 0.0 : hi.cast<double>();
        if (!hi.is_none() && !(fh > 0.0)) throw py::value_error("SSBBank: hi must lie in (lo, 0.5 / decim]");
        const std::vector<double> f = to_bfos(bfo, (size_t)nchan);
        const std::vector<int> sd = to_sides(sideband, (size_t)nchan);
        if (!taps.is_none()) {
            if (!ntaps.is_none()) throw py::value_error("SSBBank: ntaps or taps, not both");
            std::vector<float> p = to_fvec(taps);
            check(ldsp_ssbbank_create_taps((unsigned)nchan, (unsigned)decim, p.data(), (unsigned)p.size(), lo, fh, f.data(),
                                           sd.data(), q.out()));
        } else {
            const long n = ntaps.is_none() ? 0 : ntaps.cast<long>();
            if (!ntaps.is_none() && (n < 1 || n > 1025)) throw py::value_error("SSBBank: ntaps must lie in 1 .. 1025");
            check(ldsp_ssbbank_create((unsigned)nchan, (unsigned)decim, lo, fh, (unsigned)n, as, f.data(), sd.data(), q.out()));
        }
        check(ldsp_ssbbank_get_info(q, &C, &D, &L, nullptr));
    }
    void reset() { check(ldsp_ssbbank_reset(q)); }
    double lo()
    {
        double v;
        check(ldsp_ssbbank_get_band(q, &v, nullptr));
        return v;
    }
    double hi()
    {
        double v;
        check(ldsp_ssbbank_get_band(q, nullptr, &v));
        return v;
    }
    py::array_t<float> taps()
    {
        py::array_t<float> p(L);
        check(ldsp_ssbbank_get_taps(q, p.mutable_data(), nullptr));
        return p;
    }
    py::array_t<cf> row_taps()
    {
        py::array_t<cf> g({(py::ssize_t)C, (py::ssize_t)L});
        check(ldsp_ssbbank_get_taps(q, nullptr, reinterpret_cast<float*>(g.mutable_data())));
        return g;
    }
    py::array_t<uint32_t> words()
    {
        py::array_t<uint32_t> w(C);
        check(ldsp_ssbbank_get_words(q, w.mutable_data()));
        return w;
    }
    py::array_t<double> get_bfo()
    {
        py::array_t<double> f(C);
        check(ldsp_ssbbank_get_bfo(q, f.mutable_data()));
        return f;
    }
    void set_bfo(const py::object& o)
    {
        const std::vector<double> f = to_bfos(o, C);
        check(ldsp_ssbbank_set_bfo(q, f.data()));
    }
    py::list get_sideband()
    {
        std::vector<int> s(C);
        check(ldsp_ssbbank_get_sideband(q, s.data()));
        py::list l;
        for (int v : s) l.append(py::str(v > 0 ? "usb" : "lsb"));
        return l;
    }
    void set_sideband(const py::object& o)
    {
        const std::vector<int> s = to_sides(o, C);
        check(ldsp_ssbbank_set_sideband(q, s.data()));
    }
    unsigned skip()
    {
        unsigned s;
        check(ldsp_ssbbank_get_info(q, nullptr, nullptr, nullptr, &s));
        return s;
    }
    size_t tile()
    {
        size_t f = 0;
        check(ldsp_debug_ssbbank_tile(D, L, &f));
        return f;
    }
    size_t num_outputs(size_t K)
    {
        size_t c = 0;
        check(ldsp_ssbbank_num_outputs(q, K, &c));
        return c;
    }
    void seek(uint64_t T) { check(ldsp_debug_ssbbank_seek(q, T)); }
    py::object call(const py::handle& x)
    {
        return run_from_rows(q.get(), in_rows(x, Kind::c64, C, "SSBBank", true, Strided::refuse), Kind::f32, C,
                             ldsp_ssbbank_num_outputs, ldsp_ssbbank_execute);
    }
};

// ------------------------------------------------------------------ AudioBank (liquid: iirfilt_rrrf + resamp_rrrf per row)
// De-emphasis and arbitrary-rate resampler over bank rows (ldsp.h): float32[nchan, K]
// -> float32[nchan, nout] (int16 with pcm16).  A device tensor whose columns are
// one sample apart and whose rows do not overlap (an FMBank output, a block of
// rows or a range of columns of one) is read in place.
struct AudioBank {
    Handle<ldsp_audiobank_t, ldsp_audiobank_destroy> q;
    unsigned C = 0, m = 0, npfb = 0;
    float rate;
    bool pcm;
    AudioBank(int nchan, float rate_, int len, const py::object& fc, float as, int nfilter, const py::object& deemph,
              double tau, bool pcm16)
        : rate(rate_), pcm(pcm16)
    {
        if (nchan < 0) throw py::value_error("AudioBank: nchan must lie in 1 .. 256");
        if (len < 0) throw py::value_error("AudioBank: len must be >= 1");
        if (nfilter < 0) throw py::value_error("AudioBank: nfilter must be >= 1");
        const float c = fc.is_none() ? (float)(0.45 * (double)std::min(rate, 1.0f)) : fc.cast<float>();
        float sr = 0.0f;
        if (!deemph.is_none()) {
            sr = deemph.cast<float>();
            if (!(sr > 0.0f)) throw py::value_error("AudioBank: deemphasis (the rows' sample rate) must be > 0");
        }
        check(ldsp_audiobank_create((unsigned)nchan, rate, (unsigned)len, c, as, (unsigned)nfilter, sr, tau,
                                    pcm16 ? 1 : 0, q.out()));
        m = (unsigned)len;
        check(ldsp_audiobank_get_info(q, &C, &npfb, nullptr, nullptr, nullptr));
    }
    void reset() { check(ldsp_audiobank_reset(q)); }
    uint32_t step()
    {
        uint32_t v;
        check(ldsp_audiobank_get_info(q, nullptr, nullptr, &v, nullptr, nullptr));
        return v;
    }
    uint32_t phase()
    {
        uint32_t v;
        check(ldsp_audiobank_get_info(q, nullptr, nullptr, nullptr, &v, nullptr));
        return v;
    }
    py::array_t<float> taps()
    {
        unsigned n = 0;
        check(ldsp_audiobank_get_taps(q, nullptr, 0, &n));
        py::array_t<float> h(n);
        check(ldsp_audiobank_get_taps(q, h.mutable_data(), n, nullptr));
        return h;
    }
    py::object deemphasis()
    {
        float sr;
        check(ldsp_audiobank_get_coefs(q, nullptr, nullptr, &sr, nullptr));
        return sr > 0.0f ? py::object(py::float_(sr)) : py::object(py::none());
    }
    double tau()
    {
        double t;
        check(ldsp_audiobank_get_coefs(q, nullptr, nullptr, nullptr, &t));
        return t;
    }
    py::tuple coefs()
    {
        py::array_t<float> c(2);
        check(ldsp_audiobank_get_coefs(q, c.mutable_data(), c.mutable_data() + 1, nullptr, nullptr));
        return py::make_tuple(c[py::int_(0)], c[py::int_(1)]);
    }
    float get_scale() { return get_value<float>(ldsp_audiobank_get_scale, q); }
    void set_scale(float s) { check(ldsp_audiobank_set_scale(q, s)); }
    size_t tile()
    {
        size_t t = 0;
        check(ldsp_debug_audiobank_tile(q, &t));
        return t;
    }
    size_t num_outputs(size_t K)
    {
        size_t c = 0;
        check(ldsp_audiobank_num_outputs(q, K, &c));
        return c;
    }
    py::object call(const py::handle& x)
    {
        return run_from_rows(q.get(), in_rows(x, Kind::f32, C, "AudioBank", true, Strided::refuse),
                             pcm ? Kind::i16 : Kind::f32, C, ldsp_audiobank_num_outputs, ldsp_audiobank_execute);
    }
};

// ------------------------------------------------------------------ Synthesizer (no reference counterpart)
// Polyphase synthesis bank (ldsp.h): complex64[nchan, K] -> complex64[K * interp],
// row k mixed up to k / nchan.  A device tensor whose columns are contiguous (a
// block of rows or a range of columns of a Channelizer output) is read in place.
struct Synthesizer {
    Handle<ldsp_synth_t, ldsp_synth_destroy> q;
    unsigned M = 0, D = 0, L = 0;
    Synthesizer(int nchan, const py::object& interp, int m, const py::object& fc, float as, const py::object& taps)
    {
        if (nchan < 0) throw py::value_error("Synthesizer: nchan must be a power of two, at least 4");
        const int d = interp.is_none() ? nchan / 2 : interp.cast<int>();
        if (d < 0) throw py::value_error("Synthesizer: interp must be nchan or nchan // 2");
        if (!taps.is_none()) {
            std::vector<float> g = to_fvec(taps);
            check(ldsp_synth_create_taps((unsigned)nchan, (unsigned)d, g.data(), (unsigned)g.size(), q.out()));
        } else {
            if (m < 0) throw py::value_error("Synthesizer: m must be >= 1");
            const float f = opt_cutoff(fc, "Synthesizer");    // the C ABI's default: 1 / nchan or 0.5 / nchan
            check(ldsp_synth_create((unsigned)nchan, (unsigned)d, (unsigned)m, f, as, q.out()));
        }
        check(ldsp_synth_get_info(q, &M, &D, &L));
    }
    void reset() { check(ldsp_synth_reset(q)); }
    py::array_t<float> taps()
    {
        py::array_t<float> g(L);
        check(ldsp_synth_get_taps(q, g.mutable_data()));
        return g;
    }
    float get_scale() { return get_value<float>(ldsp_synth_get_scale, q); }
    void set_scale(float s) { check(ldsp_synth_set_scale(q, s)); }
    size_t tile()
    {
        size_t f = 0;
        check(ldsp_debug_synth_tile(M, D, &f));
        return f;
    }
    py::array_t<double> centers() { return wrapped_centers(M); }
    size_t num_outputs(size_t K)
    {
        size_t n = 0;
        check(ldsp_synth_num_outputs(q, K, &n));
        return n;
    }
    py::object call(const py::handle& x)
    {
        return run_from_rows(q.get(), in_rows(x, Kind::c64, M, "Synthesizer", false, Strided::copy), Kind::c64, -1,
                             ldsp_synth_num_outputs, ldsp_synth_execute);
    }
};

// ------------------------------------------------------------------ Spectrogram (no reference counterpart)
// Streaming Welch periodogram (ldsp.h): complex64[n] -> float32[rows, nfft], row
// r the mean of `average` transforms' power per bin in FFT order, plus a running
// float64 mean of every transform (psd).
struct Spectrogram {
    Handle<ldsp_spgram_t, ldsp_spgram_destroy> q;
    unsigned N = 0, W = 0, D = 0, A = 0;
    Spectrogram(long nfft, const py::object& window, const py::object& window_len, const py::object& delay,
                long average)
    {
        if (nfft < 0) throw py::value_error("Spectrogram: nfft must be a power of two");
        const long wl = window_len.is_none() ? nfft : window_len.cast<long>();
        if (wl < 0) throw py::value_error("Spectrogram: window_len must lie in 1 .. nfft");
        const long d = delay.is_none() ? std::max(wl / 2, 1L) : delay.cast<long>();
        if (d < 0) throw py::value_error("Spectrogram: delay must be at least 1");
        if (average < 0) throw py::value_error("Spectrogram: average must be at least 1");
        if (py::isinstance<py::str>(window)) {
            const std::string name = window.cast<std::string>();
            int wt = -1;
            if (name == "rect") wt = LDSP_WIN_RECT;
            else if (name == "hann") wt = LDSP_WIN_HANN;
            else if (name == "hamming") wt = LDSP_WIN_HAMMING;
            else if (name == "blackmanharris") wt = LDSP_WIN_BLACKMANHARRIS;
            check(ldsp_spgram_create((unsigned)nfft, wt, (unsigned)wl, (unsigned)d, (unsigned)average, q.out()));
        } else {
            std::vector<float> w = to_fvec(window);
            if ((long)w.size() != wl) throw py::value_error("Spectrogram: the window array's length must be window_len");
            check(ldsp_spgram_create_window((unsigned)nfft, w.data(), (unsigned)wl, (unsigned)d, (unsigned)average, q.out()));
        }
        check(ldsp_spgram_get_info(q, &N, &W, &D, &A, nullptr, nullptr));
    }
    void reset() { check(ldsp_spgram_reset(q)); }
    void clear() { check(ldsp_spgram_clear(q)); }
    py::array_t<float> window()
    {
        py::array_t<float> w(W);
        check(ldsp_spgram_get_window(q, w.mutable_data()));
        return w;
    }
    uint64_t num_samples()
    {
        uint64_t t = 0;
        check(ldsp_spgram_get_info(q, nullptr, nullptr, nullptr, nullptr, &t, nullptr));
        return t;
    }
    uint64_t num_transforms()
    {
        uint64_t t = 0;
        check(ldsp_spgram_get_info(q, nullptr, nullptr, nullptr, nullptr, nullptr, &t));
        return t;
    }
    size_t tile()
    {
        size_t f = 0;
        check(ldsp_debug_spgram_tile(N, &f));
        return f;
    }
    py::array_t<double> freqs() { return wrapped_centers(N); }
    py::array_t<double> psd()
    {
        py::array_t<double> p(N);
        double* pp = p.mutable_data();
        int rc;
        {
            py::gil_scoped_release rel;
            rc = ldsp_spgram_get_psd(q, pp, nullptr);
        }
        check(rc);
        return p;
    }
    py::tuple num_outputs(size_t n)
    {
        size_t t = 0, r = 0;
        check(ldsp_spgram_num_outputs(q, n, &t, &r));
        return py::make_tuple(t, r);
    }
    // rows: store them and return the image; otherwise accumulate only and return the transforms taken.
    // iq16: the input is int16 (I, Q) pairs, converted by the kernel's loads (ldsp_spgram_execute_iq16)
    py::object run(const py::handle& x, bool rows, bool iq16)
    {
        const auto exec = iq16 ? ldsp_spgram_execute_iq16 : ldsp_spgram_execute;
        const CallIn in = in_1d(x, iq16 ? Kind::i16 : Kind::c64);
        size_t nt = 0, K = 0, nw = 0;
        check(ldsp_spgram_num_outputs(q, in.n, &nt, &K));
        CallOut out;
        if (rows) out = make_out(in, Kind::f32, K, N);
        invoke(in, [&](int mem, void* s) { return exec(q, in.ptr, in.n, (float*)out.ptr, N, &nw, mem, s); });
        return rows ? out.obj : py::object(py::int_(nt));
    }
    py::object call(const py::handle& x) { return run(x, true, false); }
    py::object write(const py::handle& x) { return run(x, false, false); }
    // self(bytes_to_iq(raw)) / self.write(bytes_to_iq(raw)) without the complex64
    // copy: raw as ComplexIIRFilter.from_bytes takes it
    py::object from_bytes(const py::handle& b) { return run(b, true, true); }
    py::object write_bytes(const py::handle& b) { return run(b, false, true); }
};

// SSBDemod (demod.hpp:155-187): firhilbf_create(25, 60), c2r, one sideband kept
struct SSBDemod {
    bool usb;
    Hilb h;
    explicit SSBDemod(const std::string& band) : usb(band == "usb"), h(25, 60.0f, LDSP_HILB_C2R) {}
    void reset() { check(ldsp_firhilb_reset(h.q)); }
    py::object call(const py::handle& x) { return h.run(x, Kind::c64, Kind::f32, &Hilb::same, false, usb); }
};

// HilbertTransform (utility.hpp:71-108): one firhilbf per direction, each with
// its own state.  The reference calls the 2:1 functions once per input sample
// with &y[n] / &z[n] (overrunning both buffers by one sample, keeping one of two
// interpolator outputs and feeding the decimator overlapping pairs); this class
// keeps the contract of the liquid functions it names: complex64[K] ->
// float32[2K] (interp) and float32[2K] -> complex64[K] (decim).  INTEGRATION.md.
struct HilbertTransform {
    int m;
    float as;
    std::unique_ptr<Hilb> o[4];
    HilbertTransform(int m_, float as_) : m(m_), as(as_)
    {
        get(LDSP_HILB_INTERP);
        get(LDSP_HILB_DECIM);
    }
    Hilb& get(int op)
    {
        if (!o[op]) o[op].reset(new Hilb(m, as, op));
        return *o[op];
    }
    void reset()
    {
        for (auto& h : o)
            if (h) check(ldsp_firhilb_reset(h->q));
    }
    py::object interp(const py::handle& x) { return get(LDSP_HILB_INTERP).run(x, Kind::c64, Kind::f32, &Hilb::twice); }
    py::object decim(const py::handle& x) { return get(LDSP_HILB_DECIM).run(x, Kind::f32, Kind::c64, &Hilb::half); }
    py::object r2c(const py::handle& x) { return get(LDSP_HILB_R2C).run(x, Kind::f32, Kind::c64, &Hilb::same); }
    py::object c2r(const py::handle& x) { return get(LDSP_HILB_C2R).run(x, Kind::c64, Kind::f32, &Hilb::same, true); }
    // dispatch on dtype like Delay: complex64 -> interp, float32 -> decim, anything else -> None
    py::object call(const py::handle& x)
    {
        Kind k;
        if (!kind_from_dtype(x, &k)) return py::none();
        return k == Kind::c64 ? interp(x) : decim(x);
    }
};

// bytes_to_iq (utility.hpp:61-69): bytes-like -> numpy complex64; a uint8/int16
// device tensor -> complex64 device tensor
py::object bytes_to_iq(const py::handle& b)
{
    CallIn in;          // n counts bytes here; the device of a tensor is not checked
    py::buffer_info bi;
    if (is_device_tensor(b)) {
        py::object t = py::reinterpret_borrow<py::object>(b).attr("reshape")(-1).attr("contiguous")();
        on_device(in, t, DevCheck::none);
        in.n = t.attr("numel")().cast<size_t>() * t.attr("element_size")().cast<size_t>();
    } else {
        bi = py::reinterpret_borrow<py::buffer>(b).request();
        in.ptr = bi.ptr;
        in.n = (size_t)bi.size * (size_t)bi.itemsize;
    }
    CallOut out = make_out(in, Kind::c64, in.n / 4);
    invoke(in, [&](int mem, void* s) { return ldsp_bytes_to_iq(in.ptr, in.n, out.ptr, mem, s); });
    return out.obj;
}

// distinct C++ types for the distinct Python classes
struct RealResampler : Resampler {
    RealResampler(float r, int d, float fc, float as, int nf) : Resampler(r, d, fc, as, nf, false) {}
};
struct ComplexResampler : Resampler {
    ComplexResampler(float r, int d, float fc, float as, int nf) : Resampler(r, d, fc, as, nf, true) {}
};
// RResampler / CResampler (resampler.hpp:4-70): default designs, rate only
struct RResampler : Resampler {
    explicit RResampler(float r) : Resampler(r, 0) {}
};
struct CResampler : Resampler {
    explicit CResampler(float r) : Resampler(r, 2) {}
};
struct CIIRFilter : TFIIR {
    CIIRFilter(const py::handle& b, const py::handle& a) : TFIIR(b, a, true) {}
};
struct RIIRFilter : TFIIR {
    RIIRFilter(const py::handle& b, const py::handle& a) : TFIIR(b, a, false) {}
};
template <int BT, bool CPLX>
struct PassIIR : BandIIR {
    // Lowpass / Highpass hard-code f0 = 0.1 (iirfilter.hpp:70,88,180,198)
    PassIIR(const std::string& t, int order, float fc, float ap, float as) : BandIIR(t, order, fc, 0.1f, ap, as, BT, CPLX) {}
};
template <int BT, bool CPLX>
struct BandXIIR : BandIIR {
    BandXIIR(const std::string& t, int order, float fc, float f0, float ap, float as)
        : BandIIR(t, order, fc, f0, ap, as, BT, CPLX) {}
};
struct ComplexIIRFilter : ProtoIIR {
    ComplexIIRFilter(const std::string& ft, const std::string& bt, int o, float fc, float f0, float ap, float as)
        : ProtoIIR(ft, bt, o, fc, f0, ap, as, true) {}
};
struct RealIIRFilter : ProtoIIR {
    RealIIRFilter(const std::string& ft, const std::string& bt, int o, float fc, float f0, float ap, float as)
        : ProtoIIR(ft, bt, o, fc, f0, ap, as, false) {}
};

const char* kIirDispatchDoc =
    "test hook (host logic only): (path, sect_tile, size_class, spec_W, spec_staged) of a call of n samples; path is "
    "'spec', 'seq', 'modal', 'blk' or 'scan' (ldsp_debug_iir_dispatch)";
template <typename C>
py::tuple iir_dispatch(C& c, size_t n)
{
    static const char* const names[] = {"spec", "seq", "modal", "blk", "scan"};
    int path = 0, tile = 0, z = 0, w = 0, st = 0;
    check(ldsp_debug_iir_dispatch(c.q, n, &path, &tile, &z, &w, &st));
    return py::make_tuple(names[path], tile, z, w, st != 0);
}
template <typename C>
py::tuple fir_dispatch(C& c, size_t n)
{
    static const char* const names[] = {"direct", "fft", "exact"};
    int kern = 0, points = 0, overlap = 0;
    check(ldsp_debug_fir_dispatch(c.q, n, &kern, &points, &overlap));
    return py::make_tuple(names[kern], points, overlap);
}
template <typename C>
py::tuple resamp_dispatch(C& c, size_t n)
{
    static const char* const names[] = {"tile", "direct", "staged"};
    int kern = 0, kb = 0;
    check(ldsp_debug_resamp_dispatch(c.q, n, &kern, &kb));
    return py::make_tuple(names[kern], kb);
}
const char* kFirDispatchDoc =
    "test hook (host logic only): (kernel, N, P) of a call of n samples; kernel is 'direct', 'fft' or 'exact', N the "
    "FFT window and P its overlap (ldsp_debug_fir_dispatch)";
const char* kResampDispatchDoc =
    "test hook (host logic only): (kernel, outputs per workgroup) of the next call of n samples; kernel is 'tile', "
    "'direct' or 'staged' (ldsp_debug_resamp_dispatch)";

template <typename C, typename P>
void bind_iir_common(P& c)
{
    c.def("reset", &C::reset)
        .def("freqresponse", &C::freqresponse)
        .def("__call__", &C::call)
        .def("from_bytes", &C::from_bytes, py::arg("byts"),
             "self(bytes_to_iq(byts)) in one pass: int16 (I, Q) pairs converted on load (complex filters)")
        .def_property("exact", &C::get_exact, &C::set_exact)
        .def("sos", &C::sos)
        .def("_scan_path", [](C& c, int path) { check(ldsp_debug_iir_path(c.q, path)); },
             "test hook: 0 automatic, 1 blocked scan, 2 modal scan")
        .def("_modal_info", [](C& c) {
            int ok = 0, m = 0, j = 0;
            double err = 0;
            check(ldsp_debug_iir_modal_info(c.q, &ok, &m, &j, &err));
            return py::make_tuple(ok != 0, m, j, err);
        })
        .def("_modal_grid", [](C& c, size_t n) {
            long units = 0;
            int onex = 0;
            unsigned grid = 0;
            check(ldsp_debug_iir_modal_grid(c.q, n, &units, &onex, &grid));
            return py::make_tuple(units, onex != 0, grid);
        }, py::arg("n"),
             "test hook (host logic only): (units, one-XCD mode, workgroups) of a modal-scan call of n samples "
             "(ldsp_debug_iir_modal_grid)")
        .def("_dispatch", &iir_dispatch<C>, py::arg("n"), kIirDispatchDoc);
}

template <typename C>
void bind_pass(py::module_& m, const char* name)
{
    py::class_<C> c(m, name);
    c.def(py::init<std::string, int, float, float, float>(), py::arg("filter_type") = "butter", py::arg("order"),
          py::arg("Fc"), py::arg("Ap") = 0.5f, py::arg("As") = 20.0f);
    bind_iir_common<C>(c);
}
template <typename C>
void bind_band(py::module_& m, const char* name)
{
    py::class_<C> c(m, name);
    c.def(py::init<std::string, int, float, float, float, float>(), py::arg("filter_type") = "butter",
          py::arg("order"), py::arg("Fc"), py::arg("F0"), py::arg("Ap") = 0.5f, py::arg("As") = 20.0f);
    bind_iir_common<C>(c);
}
template <typename C>
void bind_proto(py::module_& m, const char* name)
{
    py::class_<C> c(m, name);
    c.def(py::init<std::string, std::string, int, float, float, float, float>(), py::arg("filter_type") = "butter",
          py::arg("band_type") = "lowpass", py::arg("order") = 2, py::arg("Fc") = 0.2f, py::arg("F0") = 0.3f,
          py::arg("Ap") = 0.7f, py::arg("As") = 60.0)
        .def_readonly("filter_type", &C::mFt)
        .def_readonly("band_type", &C::mBt)
        .def_readonly("order", &C::mOrder)
        .def_readonly("Fc", &C::mFc)
        .def_readonly("F0", &C::mF0)
        .def_readonly("Ap", &C::mAp)
        .def_readonly("As", &C::mAs)
        .def("print", &C::print);
    bind_iir_common<C>(c);
}

const char* kResampDoc = "Arbitrary-rate polyphase resampler (liquid resamp_*), runs on the GPU.";
const char* kResampInitDoc =
    "rate: output/input rate; len: filter semi-length m (20); Fc: anti-alias cutoff; As: stop-band "
    "attenuation in dB (60); nfilter: polyphase branches (13, rounded up to a power of two)";
const char* kAgcDoc = "Automatic gain control with squelch for complex IQ (liquid agc_crcf), runs on the GPU.";

} // namespace

// the registered IIR / resampler classes as their common bases (filter_resample)
template <typename... T>
IIR* iir_of(const py::object& o)
{
    IIR* r = nullptr;
    ((r = (!r && py::isinstance<T>(o)) ? static_cast<IIR*>(&o.cast<T&>()) : r), ...);
    return r;
}
IIR& as_iir(const py::object& o)
{
    IIR* r = iir_of<ComplexIIRFilter, RealIIRFilter, CIIRFilter, RIIRFilter, PassIIR<0, true>, PassIIR<1, true>,
                    BandXIIR<2, true>, BandXIIR<3, true>, PassIIR<0, false>, PassIIR<1, false>, BandXIIR<2, false>,
                    BandXIIR<3, false>, DeemphasisFilter>(o);
    if (!r) throw py::type_error("filter_resample: iir must be one of the IIR filter classes");
    return *r;
}
Resampler& as_resampler(const py::object& o)
{
    if (py::isinstance<ComplexResampler>(o)) return o.cast<ComplexResampler&>();
    if (py::isinstance<RealResampler>(o)) return o.cast<RealResampler&>();
    if (py::isinstance<CResampler>(o)) return o.cast<CResampler&>();
    if (py::isinstance<RResampler>(o)) return o.cast<RResampler&>();
    throw py::type_error("filter_resample: resampler must be one of the resampler classes");
}

PYBIND11_MODULE(_liquiddsp, m)
{
    m.doc() = "MI355X-native replacement for python-liquiddsp's streaming DSP classes (libldsp C ABI)";
    m.attr("__backend__") = "libldsp (HIP, gfx950)";

    m.def("device_count", [] {
        int n = 0;
        check(ldsp_device_count(&n));
        return n;
    });
    m.def("_math_eval", [](int fn, uintptr_t a, uintptr_t b, uintptr_t y, size_t n, uintptr_t stream) {
        check(ldsp_debug_math_eval(fn, (const float*)a, (const float*)b, (float*)y, n, (void*)stream));
    });
    // per-kernel device timing (ldsp_profile_*): {kernel: (calls, total_ms)}
    m.def("_debug_pll_margin", [](int lb) { return ldsp_debug_pll_margin(lb); });
    m.def("_debug_walk_early", [](int on) { return ldsp_debug_walk_early(on); },
          "diagnostics: the PLL walker's early hand-off (1 on, 0 off, -1 default); returns the previous setting");
    m.def("_debug_iir_sect_trace", [](uintptr_t p) { check(ldsp_debug_iir_sect_trace((void*)p)); },
          "diagnostics: device buffer address for k_iir_sect's per-wave clocks (0 = off)");
    m.def("_profile_enable", [](bool on) { check(ldsp_profile_enable(on ? 1 : 0)); });
    m.def("_profile_reset", [] { check(ldsp_profile_reset()); });
    m.def("_profile_only", [](const std::string& k) { check(ldsp_profile_only(k.c_str())); });
    m.def("_profile_report", [] {
        size_t len = 0;
        check(ldsp_profile_report(nullptr, 0, &len));
        std::string buf(len + 1, '\0');
        check(ldsp_profile_report(&buf[0], buf.size(), &len));
        py::dict d;
        size_t pos = 0;
        while (pos < len) {
            const size_t e = buf.find('\n', pos);
            const std::string line = buf.substr(pos, (e == std::string::npos ? len : e) - pos);
            pos = (e == std::string::npos) ? len : e + 1;
            char name[200];
            long calls = 0;
            double ms = 0.0;
            if (std::sscanf(line.c_str(), "%199s %ld %lf", name, &calls, &ms) == 3)
                d[py::str(name)] = py::make_tuple(calls, ms);
        }
        return d;
    });

    // ---- CIIRFilter / RIIRFilter (wrapper.cpp:30-34, 82-86)
    {
        py::class_<CIIRFilter> c(m, "CIIRFilter");
        c.def(py::init<py::handle, py::handle>(), py::arg("Bc"), py::arg("Ac"));
        bind_iir_common<CIIRFilter>(c);
    }
    {
        py::class_<RIIRFilter> c(m, "RIIRFilter");
        c.def(py::init<py::handle, py::handle>(), py::arg("Bc"), py::arg("Ac"));
        bind_iir_common<RIIRFilter>(c);
    }
    // ---- pass / band families (wrapper.cpp:36-132)
    bind_pass<PassIIR<0, true>>(m, "CLowpassIIR");
    bind_pass<PassIIR<1, true>>(m, "CHighpassIIR");
    bind_band<BandXIIR<2, true>>(m, "CBandpassIIR");
    bind_band<BandXIIR<3, true>>(m, "CBandstopIIR");
    bind_pass<PassIIR<0, false>>(m, "RLowpassIIR");
    bind_pass<PassIIR<1, false>>(m, "RHighpassIIR");
    bind_band<BandXIIR<2, false>>(m, "RBandpassIIR");
    bind_band<BandXIIR<3, false>>(m, "RBandstopIIR");
    // ---- ComplexIIRFilter / RealIIRFilter (wrapper.cpp:134-172)
    bind_proto<ComplexIIRFilter>(m, "ComplexIIRFilter");
    bind_proto<RealIIRFilter>(m, "RealIIRFilter");

    // ---- DeemphasisFilter (wrapper.cpp:178-181)
    py::class_<DeemphasisFilter>(m, "DeemphasisFilter")
        .def(py::init<float>(), py::arg("sample_rate") = 48000)
        .def("freqresponse", &DeemphasisFilter::freqresponse)
        .def("__call__", &DeemphasisFilter::call)
        .def("_dispatch", &iir_dispatch<DeemphasisFilter>, py::arg("n"), kIirDispatchDoc)
        .def("reset", &DeemphasisFilter::reset);

    // ---- AmpModem (wrapper.cpp:189-199)
    py::class_<AmpModem>(m, "AmpModem")
        .def(py::init<float, std::string, bool>(), py::arg("modulation") = 0.75, py::arg("type") = "dsb",
             py::arg("carrier") = false)
        .def_property("modulation", &AmpModem::get_modulation, &AmpModem::set_modulation)
        .def_property("type", &AmpModem::get_type, &AmpModem::set_type)
        .def_property("carrier", &AmpModem::get_carrier, &AmpModem::set_carrier)
        .def("print", &AmpModem::print)
        .def("reset", &AmpModem::reset)
        .def("pll_state", &AmpModem::pll_state)
        .def("_walk_stats", &AmpModem::walk_stats)
        .def("_taps", &AmpModem::taps)
        .def("_walk_clocks", &AmpModem::walk_clocks)
        .def("_walk_active", &AmpModem::walk_active)
        .def("_seq_stats", &AmpModem::seq_stats)
        .def("_handoff", [](AmpModem& a, uint64_t wait_ticks, int skew) {
                 check(ldsp_debug_ampmodem_handoff(a.q, wait_ticks, skew));
             }, py::arg("wait_ticks"), py::arg("epoch_skew"),
             "test hook: the early walker's wait bound (10 ns ticks, 0 = 1 s) and a skew of the epoch it waits for "
             "(ldsp_debug_ampmodem_handoff)")
        .def("_dispatch", [](AmpModem& a, size_t n) {
                 int par = 0, bat = 0;
                 check(ldsp_debug_ampmodem_dispatch(a.q, n, &par, &bat));
                 return py::make_tuple(par ? "par" : "seq", bat != 0);
             }, py::arg("n"),
             "test hook (host logic only): ('par' | 'seq', batchable) of a call of n samples "
             "(ldsp_debug_ampmodem_dispatch)")
        .def("__call__", &AmpModem::demod);

    // ---- NCO (wrapper.cpp:201-212)
    py::class_<NCO>(m, "NCO")
        .def(py::init<std::string>(), py::arg("type") = "nco")
        .def("print", &NCO::print)
        .def_property("freq", &NCO::frequency, &NCO::set_frequency)
        .def("adjust_frequency", &NCO::adjust_frequency)
        .def("adjust_phase", &NCO::adjust_phase)
        .def_property("phase", &NCO::phase, &NCO::set_phase)
        .def("set_pll_bandwidth", &NCO::set_pll_bandwidth)
        .def("pll_step", &NCO::pll_step)
        .def("state", &NCO::state)
        .def("__call__", [](NCO& n, const py::handle& x) { return n.mix(x, false); })
        .def("mix_up", [](NCO& n, const py::handle& x) { return n.mix(x, false); })
        .def("mix_down", [](NCO& n, const py::handle& x) { return n.mix(x, true); });

    // ---- NCO mix fused into a ComplexFIRFilter (BASELINE config 3; opt-in, not in wrapper.cpp)
    m.def(
        "mix_down_filter",
        [](NCO& nco, ComplexFIRFilter& fir, const py::handle& x) {
            return run_same(x, Kind::c64, Kind::c64, [&](const void* xi, size_t n, void* yo, int mem, void* s) {
                return ldsp_nco_mix_firfilt(nco.q, fir.q, xi, n, yo, 1, mem, s);
            });
        },
        py::arg("nco"), py::arg("fir"), py::arg("x"),
        "fir(nco.mix_down(x)) in one pass: same output bits and state updates as the two calls");
    m.def(
        "mix_up_filter",
        [](NCO& nco, ComplexFIRFilter& fir, const py::handle& x) {
            return run_same(x, Kind::c64, Kind::c64, [&](const void* xi, size_t n, void* yo, int mem, void* s) {
                return ldsp_nco_mix_firfilt(nco.q, fir.q, xi, n, yo, 0, mem, s);
            });
        },
        py::arg("nco"), py::arg("fir"), py::arg("x"),
        "fir(nco.mix_up(x)) in one pass: same output bits and state updates as the two calls");

    // ---- IIR fused into the resampler (README chain's first two stages; opt-in, not in wrapper.cpp)
    m.def(
        "filter_resample",
        [](py::object iir_o, py::object rs_o, const py::handle& x) {
            IIR& iir = as_iir(iir_o);
            Resampler& rs = as_resampler(rs_o);
            if (iir.cplx != rs.cplx) throw py::value_error("filter_resample: the filter and the resampler must both be complex or both real");
            return rs.run(x, iir.q);
        },
        py::arg("iir"), py::arg("resampler"), py::arg("x"),
        "resampler(iir(x)) in one pass (the filter's outputs stay on chip when it takes the fast modal scan): "
        "same output bits and state updates as the two calls");

    // ---- many-calls: one call on each of C objects of one class, one launch per kernel
    // for all of them (ldsp_*_many; device tensors on the current device's stream)
    m.def(
        "execute_many",
        [](py::list objs, py::list xs) {
            const size_t C = py::len(objs);
            if (C == 0) return py::list();
            if (py::len(xs) != C) throw py::value_error("execute_many: one input per object");
            std::vector<CallIn> ins;
            for (size_t c = 0; c < C; c++) many_in(ins, xs[c], Kind::c64, "execute_many");
            const size_t n = ins[0].n;
            py::object o0 = objs[0];
            std::vector<const void*> xp;
            for (auto& d : ins) xp.push_back(d.ptr);
            py::list outs;
            std::vector<void*> yp;
            auto mk = [&](bool cout) {
                for (size_t c = 0; c < C; c++) {
                    CallOut o = make_out(ins[c], kind_of(cout), n);
                    yp.push_back(o.ptr);
                    outs.append(o.obj);
                }
            };
            if (py::isinstance<AGC>(o0)) {
                std::vector<ldsp_agc_t> q;
                for (size_t c = 0; c < C; c++) {
                    AGC& a = objs[c].cast<AGC&>();
                    if (a.mSquelch) throw py::value_error("execute_many: AGC with squelch on (onRise replay) not supported");
                    q.push_back(a.q);
                }
                mk(true);
                check(ldsp_agc_execute_many(q.data(), xp.data(), n, yp.data(), (int)C, ins[0].stream));
                if (n > 0) g_state_last = 7;      // as AGC.__call__
            } else if (py::isinstance<AmpModem>(o0)) {
                std::vector<ldsp_ampmodem_t> q;
                for (size_t c = 0; c < C; c++) q.push_back(objs[c].cast<AmpModem&>().q);
                mk(false);
                check(ldsp_ampmodem_demodulate_many(q.data(), xp.data(), n, yp.data(), (int)C, ins[0].stream));
            } else {
                std::vector<ldsp_iirfilt_t> q;
                bool cplx = as_iir(o0).cplx;
                for (size_t c = 0; c < C; c++) {
                    IIR& f = as_iir(objs[c]);
                    if (f.cplx != cplx) throw py::value_error("execute_many: mixed real and complex filters");
                    q.push_back(f.q);
                }
                if (!cplx) {                      // real filters take float32 inputs
                    ins.clear();
                    xp.clear();
                    for (size_t c = 0; c < C; c++) {
                        ins.push_back(in_1d(xs[c], Kind::f32));
                        xp.push_back(ins[c].ptr);
                    }
                }
                mk(cplx);
                check(ldsp_iirfilt_execute_many(q.data(), xp.data(), n, yp.data(), (int)C, ins[0].stream));
            }
            return outs;
        },
        py::arg("objects"), py::arg("inputs"),
        "[obj(x) for obj, x in zip(objects, inputs)] with one kernel launch per stage for all objects: AGC, "
        "AmpModem or IIR filter objects of one class, device tensors of equal length; same bits as the separate calls");
    m.def(
        "filter_resample_many",
        [](py::list iirs, py::list rss, py::list xs) {
            const size_t C = py::len(iirs);
            if (C == 0) return py::list();
            if (py::len(rss) != C || py::len(xs) != C) throw py::value_error("filter_resample_many: one resampler and input per filter");
            std::vector<ldsp_iirfilt_t> q;
            std::vector<ldsp_resamp_t> r;
            std::vector<CallIn> ins;
            std::vector<const void*> xp;
            bool c0 = as_resampler(rss[0]).cplx;
            for (size_t c = 0; c < C; c++) {
                IIR& f = as_iir(iirs[c]);
                Resampler& rs = as_resampler(rss[c]);
                if (f.cplx != c0 || rs.cplx != c0) throw py::value_error("filter_resample_many: mixed real and complex");
                q.push_back(f.q);
                r.push_back(rs.q);
                many_in(ins, xs[c], kind_of(c0), "filter_resample_many");
                xp.push_back(ins[c].ptr);
            }
            const size_t n = ins[0].n;
            size_t cap = 0;
            std::vector<size_t> k(C);
            for (size_t c = 0; c < C; c++) {
                check(ldsp_resamp_num_outputs(r[c], n, &k[c]));
                cap = std::max(cap, k[c]);
            }
            py::list outs;
            std::vector<void*> yp;
            for (size_t c = 0; c < C; c++) {
                CallOut o = make_out(ins[c], kind_of(c0), k[c]);
                yp.push_back(o.ptr);
                outs.append(o.obj);
            }
            std::vector<size_t> nout(C);
            check(ldsp_iirfilt_resamp_execute_many(q.data(), r.data(), xp.data(), n, yp.data(), cap, nout.data(),
                                                   (int)C, ins[0].stream));
            return outs;
        },
        py::arg("iirs"), py::arg("resamplers"), py::arg("inputs"),
        "[filter_resample(f, r, x) for f, r, x in zip(...)] with one kernel launch per stage for all channels");

    // ---- bytes_to_iq, Delay (wrapper.cpp:13, 25-28)
    m.def("bytes_to_iq", &bytes_to_iq, py::arg("byts"));
    py::class_<Delay>(m, "Delay")
        .def(py::init<int>(), py::arg("nd") = 1)
        .def_property("delay", &Delay::get_delay, &Delay::set_delay)
        .def("__call__", &Delay::call);

    // ---- SSBDemod (wrapper.cpp:269-272), HilbertTransform (wrapper.cpp:174-176)
    py::class_<SSBDemod>(m, "SSBDemod")
        .def(py::init<std::string>(), py::arg("band"))
        .def("reset", &SSBDemod::reset)
        .def("__call__", &SSBDemod::call);
    py::class_<HilbertTransform>(m, "HilbertTransform")
        .def(py::init<int, float>(), py::arg("m") = 5, py::arg("As") = 60.0f)
        .def("reset", &HilbertTransform::reset)
        .def("interp", &HilbertTransform::interp, "complex64[K] -> float32[2K] (firhilbf_interp_execute)")
        .def("decim", &HilbertTransform::decim, "float32[2K] -> complex64[K] (firhilbf_decim_execute)")
        .def("r2c", &HilbertTransform::r2c, "float32[n] -> complex64[n] (firhilbf_r2c_execute)")
        .def("c2r", &HilbertTransform::c2r, "complex64[n] -> (lower, upper) float32[n] (firhilbf_c2r_execute)")
        .def("__call__", &HilbertTransform::call);
    m.def("_hilbert_tile", [](int op) {
        size_t t = 0;
        check(ldsp_debug_firhilb_tile(op, &t));
        return t;
    }, "input samples per workgroup of the Hilbert kernel of op (0 r2c, 1 c2r, 2 decim, 3 interp)");

    // ---- Channelizer (beyond the reference: polyphase analysis filter bank)
    py::class_<Channelizer>(m, "Channelizer")
        .def(py::init<int, py::object, int, py::object, float, py::object>(), py::arg("nchan"),
             py::arg("decim") = py::none(), py::arg("m") = 6, py::arg("Fc") = py::none(), py::arg("As") = 60.0f,
             py::arg("taps") = py::none())
        .def("reset", &Channelizer::reset)
        .def("num_outputs", &Channelizer::num_outputs, py::arg("n"),
             "columns the next call returns for n input samples")
        .def_property_readonly("nchan", [](Channelizer& c) { return c.M; })
        .def_property_readonly("decim", [](Channelizer& c) { return c.D; })
        .def_property_readonly("taps", &Channelizer::taps)
        .def_property("scale", &Channelizer::get_scale, &Channelizer::set_scale)
        .def_property_readonly("skip", &Channelizer::skip, "input samples before the next call's first output")
        .def_property_readonly("tile", &Channelizer::tile, "output columns per workgroup of the kernel")
        .def_property_readonly("centers", &Channelizer::centers, "channel centres k / nchan wrapped into [-0.5, 0.5)")
        .def("from_bytes", &Channelizer::from_bytes, py::arg("byts"),
             "self(bytes_to_iq(byts)) in one pass: int16 (I, Q) pairs converted on load")
        .def("__call__", &Channelizer::call, "complex64[N] -> complex64[nchan, ncols]");

    // ---- Downconverter (liquid: nco_crcf + firdecim_crcf as one bank)
    py::class_<Downconverter>(m, "Downconverter")
        .def(py::init<py::object, int, int, py::object, float, py::object>(), py::arg("freqs"), py::arg("decim"),
             py::arg("m") = 6, py::arg("Fc") = py::none(), py::arg("As") = 60.0f, py::arg("taps") = py::none())
        .def("reset", &Downconverter::reset)
        .def("num_outputs", &Downconverter::num_outputs, py::arg("n"),
             "columns the next call returns for n input samples")
        .def("_seek", &Downconverter::seek, py::arg("T"), "test hook: reset, then stream position T (zero history)")
        .def_property_readonly("ntuners", &Downconverter::ntuners)
        .def_property_readonly("decim", [](Downconverter& c) { return c.D; })
        .def_property("freqs", &Downconverter::get_freqs, &Downconverter::set_freqs,
                      "tuner frequencies words / 2**32 wrapped into [-0.5, 0.5); setting retunes (the count may change)")
        .def_property_readonly("words", &Downconverter::words, "the 32-bit frequency words")
        .def_property_readonly("taps", &Downconverter::taps)
        .def_property("scale", &Downconverter::get_scale, &Downconverter::set_scale)
        .def_property_readonly("skip", &Downconverter::skip, "input samples before the next call's first output")
        .def_property_readonly("tile", &Downconverter::tile, "output columns per workgroup of the kernel")
        .def("from_bytes", &Downconverter::from_bytes, py::arg("byts"),
             "self(bytes_to_iq(byts)) in one pass: int16 (I, Q) pairs converted on load")
        .def("__call__", &Downconverter::call, "complex64[N] -> complex64[ntuners, ncols]");

    // ---- FMBank (beyond the reference: discriminator and decimating FIR over bank rows)
    py::class_<FMBank>(m, "FMBank")
        .def(py::init<int, float, int, int, py::object, float, py::object>(), py::arg("nchan"), py::arg("kf"),
             py::arg("decim") = 1, py::arg("m") = 6, py::arg("Fc") = py::none(), py::arg("As") = 60.0f,
             py::arg("taps") = py::none())
        .def("reset", &FMBank::reset)
        .def("num_outputs", &FMBank::num_outputs, py::arg("K"),
             "columns the next call returns for K input samples per row")
        .def_property_readonly("nchan", [](FMBank& c) { return c.C; })
        .def_property_readonly("kf", [](FMBank& c) { return c.kf; })
        .def_property_readonly("decim", [](FMBank& c) { return c.D; })
        .def_property_readonly("taps", &FMBank::taps, "the prototype; empty for the discriminator alone")
        .def_property("scale", &FMBank::get_scale, &FMBank::set_scale)
        .def_property_readonly("skip", &FMBank::skip, "input samples per row before the next call's first output")
        .def_property_readonly("tile", &FMBank::tile, "output columns per workgroup of the kernel")
        .def("__call__", &FMBank::call, "complex64[nchan, K] -> float32[nchan, ncols]");

    // ---- SquelchBank (beyond the reference: per-row level and squelch gate over bank rows)
    py::class_<SquelchBank>(m, "SquelchBank")
        .def(py::init<int, int, py::object, double, int>(), py::arg("nchan"), py::arg("block") = 1024,
             py::arg("threshold") = -30.0, py::arg("bandwidth") = 0.25, py::arg("timeout") = 4)
        .def("reset", &SquelchBank::reset, "the initial state; the thresholds stay")
        .def("num_outputs", &SquelchBank::num_outputs, py::arg("K"),
             "blocks the next call returns for K input samples per row")
        .def_property_readonly("nchan", [](SquelchBank& c) { return c.C; })
        .def_property_readonly("block", [](SquelchBank& c) { return c.B; })
        .def_property_readonly("bandwidth", [](SquelchBank& c) { return c.alpha; })
        .def_property_readonly("timeout", [](SquelchBank& c) { return c.tmo; }, "in blocks")
        .def_property("threshold", &SquelchBank::get_threshold, &SquelchBank::set_threshold,
                      "dB per row; set with a scalar or nchan values, from the next block on")
        .def_property_readonly("threshold_linear", &SquelchBank::threshold_linear,
                               "the float32 values the level is compared with")
        .def_property_readonly("fill", &SquelchBank::fill, "samples per row carried to the next call")
        .def_property_readonly("tile", &SquelchBank::tile, "blocks per workgroup of the power kernel")
        .def_property_readonly("status", [](SquelchBank& c) { return c.last_status; },
                               "the last call's uint8[nchan, nblocks], liquid's squelch codes; None before the first")
        .def_property_readonly("level", [](SquelchBank& c) { return c.last_level; },
                               "the last call's float32[nchan, nblocks], linear power; None before the first")
        .def_property_readonly("state", &SquelchBank::state, "(mode, timer, smoothed power) per row after the last call")
        .def("measure", &SquelchBank::measure, py::arg("x"),
             "complex64[nchan, K] -> (status, level); advances the stream, writes no rows")
        .def("__call__", &SquelchBank::call,
             "complex64[nchan, K] -> complex64[nchan, nblocks * block]: the stream's whole blocks, closed ones zeroed");

    // ---- AGCBank (beyond the reference: look-ahead hang AGC over bank rows)
    py::class_<AGCBank>(m, "AGCBank")
        .def(py::init<int, int, py::object, double, int, double, bool>(), py::arg("nchan"), py::arg("block") = 256,
             py::arg("target") = -12.0, py::arg("max_gain") = 60.0, py::arg("hang") = 8, py::arg("decay") = 0.5,
             py::arg("complex") = false)
        .def("reset", &AGCBank::reset, "the initial state")
        .def("num_outputs", &AGCBank::num_outputs, py::arg("K"),
             "samples per row the next call returns for K input samples per row")
        .def_property_readonly("nchan", [](AGCBank& c) { return c.C; })
        .def_property_readonly("block", [](AGCBank& c) { return c.B; })
        .def_property_readonly("hang", [](AGCBank& c) { return c.H; }, "in blocks")
        .def_property_readonly("decay", [](AGCBank& c) { return c.decay; }, "dB per block")
        .def_property_readonly("max_gain", [](AGCBank& c) { return c.max_gain; }, "dB")
        .def_property_readonly("complex", [](AGCBank& c) { return c.cplx; })
        .def_property_readonly("target", &AGCBank::target, "dB re amplitude 1, per row")
        .def_property_readonly("fill", &AGCBank::fill, "samples per row carried to the next call")
        .def_property_readonly("state", &AGCBank::state,
                               "(level, the last hang peaks, the two boundary gains) per row after the last call")
        .def_property_readonly("peak_q", [](AGCBank& c) { return c.last_peak; },
                               "the last call's int32[nchan, tracked], units of 2^-24 octave; None before the first")
        .def_property_readonly("gain_q", [](AGCBank& c) { return c.last_gain; },
                               "the last call's int32[nchan, tracked], units of 2^-24 octave; None before the first")
        .def_property_readonly("gain_db", &AGCBank::gain_db, "gain_q in dB, float32")
        .def("__call__", &AGCBank::call,
             "float32 or complex64 [nchan, K] -> the same kind [nchan, emitted * block]: the stream one block behind");

    // ---- ToneBank (beyond the reference: per-row tone detector and tone squelch over bank rows)
    py::class_<ToneBank>(m, "ToneBank")
        .def(py::init<int, py::object, int, std::string, double, float, int, py::object>(), py::arg("nchan"),
             py::arg("tones"), py::arg("block") = 4096, py::arg("window") = "hann", py::arg("dominance") = 8.0,
             py::arg("floor") = 0.0f, py::arg("hold") = 1, py::arg("want") = py::none())
        .def("reset", &ToneBank::reset, "the initial state; the settings stay")
        .def("num_outputs", &ToneBank::num_outputs, py::arg("K"),
             "blocks the next call returns for K input samples per row")
        .def_property_readonly("nchan", [](ToneBank& c) { return c.C; })
        .def_property_readonly("ntones", [](ToneBank& c) { return c.F; })
        .def_property_readonly("block", [](ToneBank& c) { return c.B; })
        .def_property_readonly("hold", [](ToneBank& c) { return c.hold; }, "in blocks")
        .def_property_readonly("window", [](ToneBank& c) { return c.window == LDSP_TONE_HANN ? "hann" : "rect"; })
        .def_property_readonly("tones", &ToneBank::tones, "cycles per row sample")
        .def_property_readonly("tables", &ToneBank::tables,
                               "float32[2, ntones, block]: the cosine and sine tables, window and scale folded in")
        .def_property_readonly("window_sum", &ToneBank::sumw, "sum of the window, float64")
        .def_property("want", &ToneBank::get_want, &ToneBank::set_want,
                      "the tone that opens each row, -1 for any; set with a scalar or nchan values, from the next block on")
        .def_property("dominance", &ToneBank::get_dominance, &ToneBank::set_dominance,
                      "the best power over the mean of the others; from the next block on")
        .def_property("floor", &ToneBank::get_floor, &ToneBank::set_floor,
                      "the power the best tone must exceed; from the next block on")
        .def_property_readonly("fill", &ToneBank::fill, "samples per row carried to the next call")
        .def_property_readonly("tile", &ToneBank::tile, "columns (row, block pairs) per workgroup of the power kernel")
        .def_property_readonly("tone", [](ToneBank& c) { return c.last_tone; },
                               "the last call's int8[nchan, nblocks]: the dominant tone or -1; None before the first")
        .def_property_readonly("power", [](ToneBank& c) { return c.last_power; },
                               "the last call's float32[nchan, nblocks, ntones]; None before the first")
        .def_property_readonly("open", [](ToneBank& c) { return c.last_open; },
                               "the last call's uint8[nchan, nblocks], 1 where the gate is open; None before the first")
        .def_property_readonly("state", &ToneBank::state,
                               "blocks since the last accepted one per row after the last call (65: none within reach)")
        .def("measure", &ToneBank::measure, py::arg("x"),
             "float32[nchan, K] -> (tone, power); advances the stream, writes no rows")
        .def("__call__", &ToneBank::call,
             "float32[nchan, K] -> float32[nchan, nblocks * block]: the stream's whole blocks, closed ones zeroed");

    // ---- StereoBank (beyond the reference: feed-forward FM stereo decoder over bank rows)
    py::class_<StereoBank>(m, "StereoBank")
        .def(py::init<int, double, int, py::object, float, float, py::object, py::object>(), py::arg("nchan"),
             py::arg("pilot"), py::arg("decim") = 1, py::arg("ntaps") = py::none(), py::arg("As") = 60.0f,
             py::arg("threshold") = 0.01f, py::arg("taps") = py::none(), py::arg("pilot_taps") = py::none())
        .def("reset", &StereoBank::reset)
        .def("num_outputs", &StereoBank::num_outputs, py::arg("K"),
             "columns the next call returns for K input samples per row")
        .def_property_readonly("nchan", [](StereoBank& c) { return c.C; })
        .def_property_readonly("decim", [](StereoBank& c) { return c.D; })
        .def_property_readonly("pilot", [](StereoBank& c) { return (double)c.w / 4294967296.0; },
                               "the pilot word / 2**32, cycles per sample")
        .def_property_readonly("word", [](StereoBank& c) { return c.w; }, "the 32-bit pilot word")
        .def_property_readonly("taps", &StereoBank::taps, "the audio prototype")
        .def_property_readonly("pilot_taps", &StereoBank::pilot_taps, "the pilot prototype")
        .def_property("threshold", &StereoBank::get_threshold, &StereoBank::set_threshold,
                      "pilot amplitude |P| above which a column is decoded in stereo; set from the next call on")
        .def_property_readonly("skip", &StereoBank::skip, "input samples per row before the next call's first output")
        .def_property_readonly("tile", &StereoBank::tile, "output columns per workgroup of the kernel")
        .def_property_readonly("pilot_level", &StereoBank::pilot_level,
                               "float32[nchan]: |P| of the last column emitted per row, 0 before any")
        .def_property_readonly("stereo", &StereoBank::stereo, "bool[nchan]: pilot_level > threshold")
        .def("__call__", &StereoBank::call, "float32[nchan, K] -> float32[nchan, 2, ncols] (left, right)");

    // ---- AMBank (beyond the reference: feed-forward coherent AM demodulator over bank rows)
    py::class_<AMBank>(m, "AMBank")
        .def(py::init<int, int, py::object, double, py::object, float, float, py::object, py::object>(), py::arg("nchan"),
             py::arg("decim") = 1, py::arg("audio") = py::none(), py::arg("carrier") = 0.004,
             py::arg("ntaps") = py::none(), py::arg("As") = 60.0f, py::arg("threshold") = 0.0f,
             py::arg("taps") = py::none(), py::arg("carrier_taps") = py::none())
        .def("reset", &AMBank::reset)
        .def("num_outputs", &AMBank::num_outputs, py::arg("K"),
             "columns the next call returns for K input samples per row")
        .def_property_readonly("nchan", [](AMBank& c) { return c.C; })
        .def_property_readonly("decim", [](AMBank& c) { return c.D; })
        .def_property_readonly("ntaps", [](AMBank& c) { return c.L; })
        .def_property_readonly("taps", &AMBank::taps, "the audio prototype h")
        .def_property_readonly("carrier_taps", &AMBank::carrier_taps, "the carrier prototype g")
        .def_property_readonly("band_taps", &AMBank::band_taps, "d = h - g as float32, the taps of the audio band")
        .def_property("threshold", &AMBank::get_threshold, &AMBank::set_threshold,
                      "carrier amplitude |Cr| above which a column is demodulated; set from the next call on")
        .def_property_readonly("skip", &AMBank::skip, "input samples per row before the next call's first output")
        .def_property_readonly("tile", &AMBank::tile, "output columns per workgroup of the kernel")
        .def_property_readonly("carrier_level", &AMBank::carrier_level,
                               "float32[nchan]: |Cr| of the last column emitted per row, 0 before any")
        .def_property_readonly("carrier_present", &AMBank::carrier_present, "bool[nchan]: carrier_level > threshold")
        .def("__call__", &AMBank::call, "complex64[nchan, K] -> float32[nchan, ncols]");

    // ---- SSBBank (beyond the reference: tuned single-sideband demodulator over bank rows)
    py::class_<SSBBank>(m, "SSBBank")
        .def(py::init<int, int, double, py::object, py::object, py::object, py::object, float, py::object>(),
             py::arg("nchan"), py::arg("decim") = 1, py::arg("lo") = 0.025, py::arg("hi") = py::none(),
             py::arg("bfo") = 0.0, py::arg("sideband") = "usb", py::arg("ntaps") = py::none(), py::arg("As") = 60.0f,
             py::arg("taps") = py::none())
        .def("reset", &SSBBank::reset)
        .def("num_outputs", &SSBBank::num_outputs, py::arg("K"),
             "columns the next call returns for K input samples per row")
        .def("_seek", &SSBBank::seek, py::arg("T"), "test hook: reset, then stream position T (zero history)")
        .def_property_readonly("nchan", [](SSBBank& c) { return c.C; })
        .def_property_readonly("decim", [](SSBBank& c) { return c.D; })
        .def_property_readonly("ntaps", [](SSBBank& c) { return c.L; })
        .def_property_readonly("lo", &SSBBank::lo, "lower band edge, cycles per row sample from the carrier")
        .def_property_readonly("hi", &SSBBank::hi, "upper band edge, cycles per row sample from the carrier")
        .def_property_readonly("taps", &SSBBank::taps, "the real low-pass prototype p")
        .def_property_readonly("row_taps", &SSBBank::row_taps, "complex64[nchan, ntaps]: the rows' band-pass taps g")
        .def_property("bfo", &SSBBank::get_bfo, &SSBBank::set_bfo,
                      "float64[nchan]: the carriers' positions in the rows; set (a scalar or one per row) from the next call on")
        .def_property_readonly("words", &SSBBank::words, "uint32[nchan]: the 32-bit BFO words")
        .def_property("sideband", &SSBBank::get_sideband, &SSBBank::set_sideband,
                      "list of 'usb' / 'lsb' per row; set (one name or one per row) from the next call on")
        .def_property_readonly("skip", &SSBBank::skip, "input samples per row before the next call's first output")
        .def_property_readonly("tile", &SSBBank::tile, "output columns per workgroup of the kernel")
        .def("__call__", &SSBBank::call, "complex64[nchan, K] -> float32[nchan, ncols]");

    // ---- AudioBank (beyond the reference: de-emphasis and resampler over bank rows)
    py::class_<AudioBank>(m, "AudioBank")
        .def(py::init<int, float, int, py::object, float, int, py::object, double, bool>(), py::arg("nchan"),
             py::arg("rate"), py::arg("len") = 20, py::arg("Fc") = py::none(), py::arg("As") = 60.0f,
             py::arg("nfilter") = 13, py::arg("deemphasis") = py::none(), py::arg("tau") = 75e-6,
             py::arg("pcm16") = false)
        .def("reset", &AudioBank::reset)
        .def("num_outputs", &AudioBank::num_outputs, py::arg("K"),
             "outputs per row the next call returns for K input samples per row")
        .def_property_readonly("nchan", [](AudioBank& c) { return c.C; })
        .def_property_readonly("rate", [](AudioBank& c) { return c.rate; })
        .def_property_readonly("len", [](AudioBank& c) { return c.m; })
        .def_property_readonly("nfilter", [](AudioBank& c) { return c.npfb; }, "after liquid's rounding to a power of two")
        .def_property_readonly("step", &AudioBank::step)
        .def_property_readonly("phase", &AudioBank::phase)
        .def_property_readonly("taps", &AudioBank::taps, "the prototype, 2 len nfilter + 1 taps")
        .def_property_readonly("deemphasis", &AudioBank::deemphasis, "the rows' sample rate in Hz; None: no de-emphasis")
        .def_property_readonly("tau", &AudioBank::tau)
        .def_property_readonly("coefs", &AudioBank::coefs, "(b0, a) of the de-emphasis as float32")
        .def_property_readonly("pcm16", [](AudioBank& c) { return c.pcm; })
        .def_property("scale", &AudioBank::get_scale, &AudioBank::set_scale)
        .def_property_readonly("tile", &AudioBank::tile, "outputs per workgroup of the kernel")
        .def("__call__", &AudioBank::call, "float32[nchan, K] -> float32[nchan, nout] (int16 with pcm16)");

    // ---- Synthesizer (beyond the reference: polyphase synthesis filter bank)
    py::class_<Synthesizer>(m, "Synthesizer")
        .def(py::init<int, py::object, int, py::object, float, py::object>(), py::arg("nchan"),
             py::arg("interp") = py::none(), py::arg("m") = 6, py::arg("Fc") = py::none(), py::arg("As") = 60.0f,
             py::arg("taps") = py::none())
        .def("reset", &Synthesizer::reset)
        .def("num_outputs", &Synthesizer::num_outputs, py::arg("K"), "samples a call of K columns returns")
        .def_property_readonly("nchan", [](Synthesizer& c) { return c.M; })
        .def_property_readonly("interp", [](Synthesizer& c) { return c.D; })
        .def_property_readonly("taps", &Synthesizer::taps)
        .def_property("scale", &Synthesizer::get_scale, &Synthesizer::set_scale)
        .def_property_readonly("tile", &Synthesizer::tile, "input columns per workgroup of the kernel")
        .def_property_readonly("centers", &Synthesizer::centers, "row centres k / nchan wrapped into [-0.5, 0.5)")
        .def("__call__", &Synthesizer::call, "complex64[nchan, K] -> complex64[K * interp]");

    // ---- Spectrogram (beyond the reference: streaming Welch periodogram)
    py::class_<Spectrogram>(m, "Spectrogram")
        .def(py::init<long, py::object, py::object, py::object, long>(), py::arg("nfft"), py::arg("window") = "hann",
             py::arg("window_len") = py::none(), py::arg("delay") = py::none(), py::arg("average") = 1)
        .def("reset", &Spectrogram::reset, "zero the history, the counts, the unfinished row and the accumulator")
        .def("clear", &Spectrogram::clear, "zero the accumulator and num_transforms only")
        .def("num_outputs", &Spectrogram::num_outputs, py::arg("n"),
             "(transforms, rows) the next call takes / returns for n input samples")
        .def("write", &Spectrogram::write, "accumulate only; returns the transforms taken")
        .def("from_bytes", &Spectrogram::from_bytes, py::arg("byts"),
             "self(bytes_to_iq(byts)) in one pass: int16 (I, Q) pairs converted on load")
        .def("write_bytes", &Spectrogram::write_bytes, py::arg("byts"),
             "self.write(bytes_to_iq(byts)) in one pass: int16 (I, Q) pairs converted on load")
        .def_property_readonly("nfft", [](Spectrogram& c) { return c.N; })
        .def_property_readonly("window", &Spectrogram::window)
        .def_property_readonly("window_len", [](Spectrogram& c) { return c.W; })
        .def_property_readonly("delay", [](Spectrogram& c) { return c.D; })
        .def_property_readonly("average", [](Spectrogram& c) { return c.A; })
        .def_property_readonly("num_samples", &Spectrogram::num_samples, "input samples since creation or reset()")
        .def_property_readonly("num_transforms", &Spectrogram::num_transforms,
                               "transforms in psd: since creation, reset() or clear()")
        .def_property_readonly("psd", &Spectrogram::psd, "float64[nfft]: mean power per bin over num_transforms")
        .def_property_readonly("freqs", &Spectrogram::freqs, "bin centres k / nfft wrapped into [-0.5, 0.5)")
        .def_property_readonly("tile", &Spectrogram::tile, "transforms per workgroup of the kernel")
        .def("__call__", &Spectrogram::call, "complex64[n] -> float32[rows, nfft]");

    // ---- FreqDem (wrapper.cpp:183-187), BroadcastAM (wrapper.cpp:259-262)
    py::class_<FreqDem>(m, "FreqDem")
        .def(py::init<float>())
        .def("reset", &FreqDem::reset)
        .def("print", &FreqDem::print)
        .def("__call__", &FreqDem::call);
    py::class_<BroadcastAM>(m, "BroadcastAM")
        .def(py::init<int>(), py::arg("slen") = 25)
        .def("reset", &BroadcastAM::reset)
        .def_property("exact", &BroadcastAM::get_exact, &BroadcastAM::set_exact)
        .def("__call__", &BroadcastAM::call);

    // ---- FMStereo (wrapper.cpp:264-267)
    py::class_<FMStereo>(m, "FMStereo")
        .def(py::init<float, float>(), py::arg("iq_rate") = 600000.0f, py::arg("pcm_rate") = 48000.0f)
        .def("reset", &FMStereo::reset)
        .def("state", &FMStereo::state)
        .def("__call__", &FMStereo::call);

    // ---- RResampler / CResampler (wrapper.cpp:15-23)
    py::class_<RResampler>(m, "RResampler")
        .def(py::init<float>(), py::arg("rate"))
        .def("reset", &RResampler::reset)
        .def("__call__", &RResampler::call);
    py::class_<CResampler>(m, "CResampler")
        .def(py::init<float>(), py::arg("rate"))
        .def("reset", &CResampler::reset)
        .def("__call__", &CResampler::call);

    // ---- RealResampler / ComplexResampler (wrapper.cpp:214-226)
    py::class_<RealResampler>(m, "RealResampler", kResampDoc)
        .def(py::init<float, int, float, float, int>(), py::arg("rate"), py::arg("len") = 20, py::arg("Fc"),
             py::arg("As") = 60.0f, py::arg("nfilter") = 13, kResampInitDoc)
        .def("print", &RealResampler::print)
        .def("reset", &RealResampler::reset)
        .def("__call__", &RealResampler::call)
        .def("_dispatch", &resamp_dispatch<RealResampler>, py::arg("n"), kResampDispatchDoc)
        .def_property("rate", &RealResampler::get_rate, &RealResampler::set_rate);
    py::class_<ComplexResampler>(m, "ComplexResampler", kResampDoc)
        .def(py::init<float, int, float, float, int>(), py::arg("rate"), py::arg("len") = 20, py::arg("Fc"),
             py::arg("As") = 60.0f, py::arg("nfilter") = 13, kResampInitDoc)
        .def("print", &ComplexResampler::print)
        .def("reset", &ComplexResampler::reset)
        .def("__call__", &ComplexResampler::call)
        .def("_dispatch", &resamp_dispatch<ComplexResampler>, py::arg("n"), kResampDispatchDoc)
        .def_property("rate", &ComplexResampler::get_rate, &ComplexResampler::set_rate);

    // ---- AGC (wrapper.cpp:228-242)
    py::class_<AGC>(m, "AGC", kAgcDoc)
        .def(py::init<>())
        .def_property("squelch", &AGC::get_squelch, &AGC::set_squelch)
        .def_property("threshold", &AGC::get_threshold, &AGC::set_threshold)
        .def_property("bandwidth", &AGC::get_bandwidth, &AGC::set_bandwidth)
        .def_property("level", &AGC::get_level, &AGC::set_level)
        .def_property("level_dB", &AGC::get_rssi, &AGC::set_rssi)
        .def_property("lock", &AGC::get_lock, &AGC::set_lock)
        .def_property("gain", &AGC::get_gain, &AGC::set_gain)
        .def_property("scale", &AGC::get_scale, &AGC::set_scale)
        .def_property_readonly("status", &AGC::status)
        .def("_tsa_perturb", [](AGC& a, bool on) { check(ldsp_debug_agc_tsa_perturb(a.q, on ? 1 : 0)); },
             "test hook: small calls re-run every chunk in-kernel (ldsp_debug_agc_tsa_perturb)")
        .def("_perturb", [](AGC& a, bool on) { check(ldsp_debug_agc_perturb(a.q, on ? 1 : 0)); },
             "test hook: chunk-parallel calls start every odd chunk 1 ulp off (ldsp_debug_agc_perturb)")
        .def("_rounds", [](AGC& a, int r) { check(ldsp_debug_agc_rounds(a.q, r)); },
             "test hook: repair rounds before the verifier (-1 default; ldsp_debug_agc_rounds)")
        .def("_reruns", [](AGC& a) {
            unsigned rf = 0, vf = 0;
            check(ldsp_debug_agc_reruns(a.q, &rf, &vf));
            return py::make_tuple(rf, vf);
        }, "test hook: (repair-round, verifier) chunk re-runs since creation (ldsp_debug_agc_reruns)")
        .def("_dispatch", [](AGC& a, size_t n) {
            static const char* const names[] = {"seq", "small", "par"};
            int path = 0, W = 0, Wa = 0, C = 0, spec = 0;
            long hl = 0, hv = 0;
            check(ldsp_debug_agc_dispatch(a.q, n, &path, &W, &Wa, &C, &hl, &hv, &spec));
            return py::make_tuple(names[path], W, Wa, C, hl, hv, spec != 0);
        }, py::arg("n"),
             "test hook (host logic only): (path, W, Wa, C, hist_len, hist_valid, speculative) of the next call of n "
             "samples; path is 'seq', 'small' or 'par' (ldsp_debug_agc_dispatch)")
        .def("_tsa_reruns", [](AGC& a) {
            unsigned c = 0;
            check(ldsp_debug_agc_tsa_reruns(a.q, &c));
            return c;
        })
        .def_property(
            "onRise", [](AGC& a) { return a.mOnRise; }, [](AGC& a, py::object f) { a.mOnRise = f; })
        .def("print", &AGC::print)
        .def("reset", &AGC::reset)
        .def("__call__", &AGC::call);

    // ---- FIR family (wrapper.cpp:244-257) + the new ComplexFIRFilter
    py::class_<RealFIRFilter>(m, "RealFIRFilter")
        .def(py::init<py::handle>(), py::arg("h"))
        .def("freqresponse", &RealFIRFilter::freqresponse)
        .def("__call__", &RealFIRFilter::call)
        .def("reset", &RealFIRFilter::reset)
        .def_property("exact", &RealFIRFilter::get_exact, &RealFIRFilter::set_exact)
        .def_property("mode", &RealFIRFilter::get_mode, &RealFIRFilter::set_mode)
        .def("_dispatch", &fir_dispatch<RealFIRFilter>, py::arg("n"), kFirDispatchDoc)
        .def_property_readonly("taps", &RealFIRFilter::taps);
    py::class_<ComplexFIRFilter>(m, "ComplexFIRFilter")
        .def(py::init<py::handle>(), py::arg("h"))
        .def("freqresponse", &ComplexFIRFilter::freqresponse)
        .def("__call__", &ComplexFIRFilter::call)
        .def("reset", &ComplexFIRFilter::reset)
        .def_property("exact", &ComplexFIRFilter::get_exact, &ComplexFIRFilter::set_exact)
        .def_property("mode", &ComplexFIRFilter::get_mode, &ComplexFIRFilter::set_mode)
        .def("_dispatch", &fir_dispatch<ComplexFIRFilter>, py::arg("n"), kFirDispatchDoc)
        .def_property_readonly("taps", &ComplexFIRFilter::taps);
    py::class_<RealDCBlocker>(m, "RealDCBlocker")
        .def(py::init<int, float>(), py::arg("slen") = 25, py::arg("As") = 20.0f)
        .def("freqresponse", &RealDCBlocker::freqresponse)
        .def("__call__", &RealDCBlocker::call)
        .def("reset", &RealDCBlocker::reset)
        .def_property("exact", &RealDCBlocker::get_exact, &RealDCBlocker::set_exact)
        .def_property("mode", &RealDCBlocker::get_mode, &RealDCBlocker::set_mode)
        .def_property_readonly("taps", &RealDCBlocker::taps);
    py::class_<RealKaiserBessel>(m, "RealKaiserBessel")
        .def(py::init<int, float, float, float>(), py::arg("flen") = 25, py::arg("Fc"), py::arg("As") = 20.0f,
             py::arg("offset") = 0.0f)
        .def("freqresponse", &RealKaiserBessel::freqresponse)
        .def("__call__", &RealKaiserBessel::call)
        .def("reset", &RealKaiserBessel::reset)
        .def_property("exact", &RealKaiserBessel::get_exact, &RealKaiserBessel::set_exact)
        .def_property("mode", &RealKaiserBessel::get_mode, &RealKaiserBessel::set_mode)
        .def_property_readonly("taps", &RealKaiserBessel::taps)
        .def_property_readonly("scale", &RealKaiserBessel::get_scale);
}
