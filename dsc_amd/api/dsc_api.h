// dsc_api.h — header-only C++ wrapper over the C ABI in include/dsc_mi355x.h.
//
// Mirror of the reference's dsc/api/dsc_api.h: `dsc::init`, RAII `dsc::tensor<T>`, the arithmetic operators, `dsc::pow`,
// `dsc::cos .. sqrt`, `dsc::i0`, `dsc::clip`, `dsc::arange / randn`, `dsc::reshape / concat`, `dsc::sum`,
// `dsc::fft / ifft / rfft / irfft` (reference lines 15-21, 24-34, 36-143, 148-189, 260-319, 321-343) plus `dsc::filter_fft`, `dsc::stft / istft` `dsc::convolve / correlate`, `dsc::fft2 / ifft2 / rfft2 / irfft2` `dsc::hilbert / envelope`, `dsc::upfirdn / resample_poly / decimate / firwin`, `dsc::cumsum / diff / unwrap / phase`, `dsc::roll / flip / fftshift / ifftshift / pad` and `dsc::sumsq / rms / var / std / vdot / detrend`.  The one semantic
// difference: tensor payloads live in HBM, so construction from host data and `to_host()`
// copy through dsc_copy_from_host / dsc_copy_to_host instead of dereferencing `data()`
// (reference: memcpy into x_->data, dsc_api.h:63-66).
#pragma once

#include "dsc_mi355x.h"

#include <cstddef>
#include <initializer_list>
#include <type_traits>
#include <vector>

// dsc_api.h:15-21
#define DSC_SLICE_ALL()                 (dsc_slice{DSC_VALUE_NONE, DSC_VALUE_NONE, 1})
#define DSC_SLICE_IDX(idx_)             (dsc_slice{(idx_), (idx_), (idx_)})      // a single element, not a slice
#define DSC_SLICE_ALL_STEP(step_)       (dsc_slice{DSC_VALUE_NONE, DSC_VALUE_NONE, (step_)})
#define DSC_SLICE_FROM(start_)          (dsc_slice{(start_), DSC_VALUE_NONE, 1})
#define DSC_SLICE_TO(stop_)             (dsc_slice{DSC_VALUE_NONE, (stop_), 1})
#define DSC_SLICE_RANGE(start_, stop_)  (dsc_slice{(start_), (stop_), 1})

namespace dsc {

static dsc_ctx *ctx = nullptr;             // dsc_api.h:26

// dsc_api.h:28-34: with scratch_mem == 0, 90 % of main_mem goes to the main arena and a
// tenth of that to scratch.
static inline void init(size_t main_mem, size_t scratch_mem = 0, int device = 0) {
    if (scratch_mem == 0) {
        main_mem = (size_t) ((double) main_mem * 0.9);
        scratch_mem = (size_t) ((double) main_mem * 0.1);
    }
    dsc_set_device(device);
    ctx = dsc_ctx_init(main_mem, scratch_mem);
}

template<typename T> struct dtype_of;
template<> struct dtype_of<float>   { static constexpr dsc_dtype value = DSC_F32; };
template<> struct dtype_of<double>  { static constexpr dsc_dtype value = DSC_F64; };
template<> struct dtype_of<dsc_c32> { static constexpr dsc_dtype value = DSC_C32; };
template<> struct dtype_of<dsc_c64> { static constexpr dsc_dtype value = DSC_C64; };

template<typename T>
class tensor {
public:
    tensor() noexcept : x_(nullptr) {}
    tensor(dsc_tensor *x) noexcept : x_(x) {}
    // host data -> new 1-D device tensor (reference: tensor(const T*, int), dsc_api.h:63-66)
    tensor(const T *host, int ne) noexcept {
        x_ = dsc_new_tensor(ctx, 1, &ne, dtype_of<T>::value, nullptr);
        dsc_copy_from_host(ctx, x_, host, (size_t) ne * sizeof(T));
    }
    // host data -> new n-D device tensor
    tensor(const T *host, std::initializer_list<int> shape) noexcept {
        int s[DSC_MAX_DIMS];
        int n = 0;
        size_t ne = 1;
        for (int d : shape) { s[n++] = d; ne *= (size_t) d; }
        x_ = dsc_new_tensor(ctx, n, s, dtype_of<T>::value, nullptr);
        dsc_copy_from_host(ctx, x_, host, ne * sizeof(T));
    }
    // {a, b, c} -> 1-D tensor of scalars; ({shape}, fill) -> constant tensor        (dsc_api.h:46-57)
    tensor(std::initializer_list<T> scalars) noexcept : tensor(std::vector<T>(scalars).data(), (int) scalars.size()) {}
    tensor(std::initializer_list<int> shape, const T fill) noexcept {
        int s[DSC_MAX_DIMS];
        int n = 0;
        size_t ne = 1;
        for (int d : shape) { s[n++] = d; ne *= (size_t) d; }
        x_ = dsc_new_tensor(ctx, n, s, dtype_of<T>::value, nullptr);
        const std::vector<T> host(ne, fill);
        dsc_copy_from_host(ctx, x_, host.data(), ne * sizeof(T));
    }
    // Copies are DEEP, as in the reference (memcpy of the payload, dsc_api.h:63-81); here the payload is copied on the
    // device: selecting everything with one full slice is dsc_tensor_get_slice's copy kernel.
    tensor(const tensor &o) noexcept : x_(o.x_ == nullptr ? nullptr : clone(o.x_)) {}
    tensor &operator=(const tensor &o) noexcept {
        if (this != &o) {
            if (x_ != nullptr) dsc_tensor_free(ctx, x_);
            x_ = o.x_ == nullptr ? nullptr : clone(o.x_);
        }
        return *this;
    }
    tensor(tensor &&o) noexcept : x_(o.x_) { o.x_ = nullptr; }
    tensor &operator=(tensor &&o) noexcept {
        if (this != &o) {
            if (x_ != nullptr) dsc_tensor_free(ctx, x_);
            x_ = o.x_;
            o.x_ = nullptr;
        }
        return *this;
    }
    ~tensor() noexcept { if (x_ != nullptr) dsc_tensor_free(ctx, x_); }

    int dim(int idx) const noexcept { return x_->shape[idx < 0 ? DSC_MAX_DIMS + idx : DSC_MAX_DIMS - x_->n_dim + idx]; }
    int size() const noexcept { return dim(0); }
    int ndim() const noexcept { return x_->n_dim; }
    int ne() const noexcept { return x_->ne; }
    dsc_dtype dtype() const noexcept { return x_->dtype; }
    dsc_tensor *raw() const noexcept { return x_; }

    // device -> host copy of the whole payload, as elements of U (e.g. dsc_c32 for an rfft result:
    // like the reference, rfft<float> returns tensor<float> whose payload is complex, dsc_api.h:333-337)
    template<typename U = T>
    std::vector<U> to_host() const {
        const size_t bytes = (size_t) x_->ne * (x_->dtype == DSC_F32 ? 4 : x_->dtype == DSC_C64 ? 16 : 8);
        std::vector<U> out(bytes / sizeof(U));
        dsc_copy_to_host(ctx, x_, out.data(), bytes);
        return out;
    }

    // dsc_api.h:148-186: element-wise operators with broadcasting; a scalar operand of the tensor's own element type is
    // wrapped into a one-element tensor (dsc_wrap_*), on either side.
    tensor operator+(const tensor &o) const noexcept { return dsc_add(ctx, x_, o.x_, nullptr); }
    tensor operator+(const T v) const noexcept { return dsc_add(ctx, x_, wrap(v).x_, nullptr); }
    friend tensor operator+(const T v, const tensor &o) noexcept { return wrap(v) + o; }
    tensor operator-(const tensor &o) const noexcept { return dsc_sub(ctx, x_, o.x_, nullptr); }
    tensor operator-(const T v) const noexcept { return dsc_sub(ctx, x_, wrap(v).x_, nullptr); }
    friend tensor operator-(const T v, const tensor &o) noexcept { return wrap(v) - o; }
    tensor operator*(const tensor &o) const noexcept { return dsc_mul(ctx, x_, o.x_, nullptr); }
    tensor operator*(const T v) const noexcept { return dsc_mul(ctx, x_, wrap(v).x_, nullptr); }
    friend tensor operator*(const T v, const tensor &o) noexcept { return wrap(v) * o; }
    tensor operator/(const tensor &o) const noexcept { return dsc_div(ctx, x_, o.x_, nullptr); }
    tensor operator/(const T v) const noexcept { return dsc_div(ctx, x_, wrap(v).x_, nullptr); }
    friend tensor operator/(const T v, const tensor &o) noexcept { return wrap(v) / o; }
    tensor &operator/=(const tensor &o) noexcept { dsc_div(ctx, x_, o.x_, x_); return *this; }     // in place: out = x
    tensor &operator*=(const tensor &o) noexcept { dsc_mul(ctx, x_, o.x_, x_); return *this; }

    // dsc_api.h:117-143: x.get(2, 3) (indexes) / x.get(DSC_SLICE_ALL(), DSC_SLICE_TO(n)) (slices) copy on the device
    template<typename... Args>
    tensor get(Args... sel) const noexcept {
        if constexpr ((std::is_same_v<Args, dsc_slice> && ...)) return dsc_tensor_get_slice(ctx, x_, (int) sizeof...(Args), sel...);
        else                                                      return dsc_tensor_get_idx(ctx, x_, (int) sizeof...(Args), ((int) sel)...);
    }
    template<typename... Args>
    tensor &set(const tensor &other, Args... sel) noexcept {
        if constexpr ((std::is_same_v<Args, dsc_slice> && ...)) dsc_tensor_set_slice(ctx, x_, other.x_, (int) sizeof...(Args), sel...);
        else                                                      dsc_tensor_set_idx(ctx, x_, other.x_, (int) sizeof...(Args), ((int) sel)...);
        return *this;
    }

    dsc_tensor *x_;

private:
    static dsc_tensor *clone(dsc_tensor *src) noexcept { return dsc_tensor_get_slice(ctx, src, 1, DSC_SLICE_ALL()); }
    static tensor wrap(const T v) noexcept {
        if constexpr (std::is_same_v<T, float>)        return dsc_wrap_f32(ctx, v);
        else if constexpr (std::is_same_v<T, double>)  return dsc_wrap_f64(ctx, v);
        else if constexpr (std::is_same_v<T, dsc_c32>) return dsc_wrap_c32(ctx, v);
        else                                           return dsc_wrap_c64(ctx, v);
    }
};

template<typename T>
static inline tensor<T> sum(const tensor<T> &x, int axis = -1, bool keep_dims = true) noexcept {            // dsc_api.h:285-290
    return dsc_sum(ctx, x.x_, nullptr, axis, keep_dims);
}
template<typename T>
static inline tensor<T> mean(const tensor<T> &x, int axis = -1, bool keep_dims = true) noexcept {
    return dsc_mean(ctx, x.x_, nullptr, axis, keep_dims);
}
template<typename T>
static inline tensor<T> max(const tensor<T> &x, int axis = -1, bool keep_dims = true) noexcept {
    return dsc_max(ctx, x.x_, nullptr, axis, keep_dims);
}
template<typename T>
static inline tensor<T> min(const tensor<T> &x, int axis = -1, bool keep_dims = true) noexcept {
    return dsc_min(ctx, x.x_, nullptr, axis, keep_dims);
}

// dsc_api.h:294-302: transpose(x) reverses the axes, transpose(x, 1, 0, ...) permutes them
template<typename T, typename... Args>
static inline tensor<T> transpose(const tensor<T> &x, Args... axes) noexcept {
    static_assert((std::is_same_v<Args, int> && ...), "axes are ints");
    if constexpr (sizeof...(Args) == 0) return dsc_transpose(ctx, x.x_, 0);
    else                                return dsc_transpose(ctx, x.x_, (int) sizeof...(Args), axes...);
}

template<typename T>
static inline tensor<T> fft(const tensor<T> &x, int n = -1, int axis = -1) noexcept { return dsc_fft(ctx, x.x_, nullptr, n, axis); }
template<typename T>
static inline tensor<T> ifft(const tensor<T> &x, int n = -1, int axis = -1) noexcept { return dsc_ifft(ctx, x.x_, nullptr, n, axis); }
template<typename T>
static inline tensor<T> rfft(const tensor<T> &x, int n = -1, int axis = -1) noexcept { return dsc_rfft(ctx, x.x_, nullptr, n, axis); }
template<typename T>
static inline tensor<T> irfft(const tensor<T> &x, int n = -1, int axis = -1) noexcept { return dsc_irfft(ctx, x.x_, nullptr, n, axis); }

// dsc_api.h:187-189: x.pow(e) is a free function here, pow(x, e) / pow(x, y)
template<typename T>
static inline tensor<T> pow(const tensor<T> &x, const tensor<T> &e) noexcept { return dsc_pow(ctx, x.x_, e.x_, nullptr); }
template<typename T>
static inline tensor<T> pow(const tensor<T> &x, const T e) noexcept { return dsc_pow(ctx, x.x_, tensor<T>({e}).x_, nullptr); }

// dsc_api.h:260-283: element-wise functions, i0, clip, arange
template<typename T> static inline tensor<T> cos(const tensor<T> &x) noexcept { return dsc_cos(ctx, x.x_, nullptr); }
template<typename T> static inline tensor<T> sin(const tensor<T> &x) noexcept { return dsc_sin(ctx, x.x_, nullptr); }
template<typename T> static inline tensor<T> sinc(const tensor<T> &x) noexcept { return dsc_sinc(ctx, x.x_, nullptr); }
template<typename T> static inline tensor<T> logn(const tensor<T> &x) noexcept { return dsc_logn(ctx, x.x_, nullptr); }
template<typename T> static inline tensor<T> log2(const tensor<T> &x) noexcept { return dsc_log2(ctx, x.x_, nullptr); }
template<typename T> static inline tensor<T> log10(const tensor<T> &x) noexcept { return dsc_log10(ctx, x.x_, nullptr); }
template<typename T> static inline tensor<T> exp(const tensor<T> &x) noexcept { return dsc_exp(ctx, x.x_, nullptr); }
template<typename T> static inline tensor<T> sqrt(const tensor<T> &x) noexcept { return dsc_sqrt(ctx, x.x_, nullptr); }
template<typename T> static inline tensor<T> i0(const tensor<T> &x) noexcept { return dsc_i0(ctx, x.x_); }
template<typename T>
static inline tensor<T> clip(const tensor<T> &x, double x_min = -__builtin_inf(), double x_max = __builtin_inf()) noexcept {
    return dsc_clip(ctx, x.x_, nullptr, x_min, x_max);
}
template<typename T>
static inline tensor<T> arange(int n) noexcept { return dsc_arange(ctx, n, dtype_of<T>::value); }
template<typename T>
static inline tensor<T> randn(std::initializer_list<int> shape) noexcept {
    const std::vector<int> s(shape);
    return dsc_randn(ctx, (int) s.size(), s.data(), dtype_of<T>::value);
}

// dsc_api.h:304-319: reshape(x, 4, -1) shares x's buffer; concat(axis, a, b, ...) copies (axis = DSC_VALUE_NONE flattens)
template<typename T, typename... Args>
static inline tensor<T> reshape(const tensor<T> &x, Args... dimensions) noexcept {
    static_assert((std::is_same_v<Args, int> && ...), "dimensions are ints");
    return dsc_reshape(ctx, x.x_, (int) sizeof...(Args), dimensions...);
}
template<typename T, typename... Args>
static inline tensor<T> concat(int axis, const tensor<T> &first, const Args &...rest) noexcept {
    return dsc_concat(ctx, axis, 1 + (int) sizeof...(Args), first.x_, rest.x_...);
}

// Section F of dsc_mi355x.h: 2-D transforms over the last two axes (numpy.fft.fft2 / ifft2 / rfft2 / irfft2, s = (n0, n1))
template<typename T>
static inline tensor<T> fft2(const tensor<T> &x, int n0 = -1, int n1 = -1) noexcept { return dsc_fft2(ctx, x.x_, nullptr, n0, n1); }
template<typename T>
static inline tensor<T> ifft2(const tensor<T> &x, int n0 = -1, int n1 = -1) noexcept { return dsc_ifft2(ctx, x.x_, nullptr, n0, n1); }
template<typename T>
static inline tensor<T> rfft2(const tensor<T> &x, int n0 = -1, int n1 = -1) noexcept { return dsc_rfft2(ctx, x.x_, nullptr, n0, n1); }
template<typename T>
static inline tensor<T> irfft2(const tensor<T> &x, int n0 = -1, int n1 = -1) noexcept { return dsc_irfft2(ctx, x.x_, nullptr, n0, n1); }

// README.md:141-163 (C++ filterFFT) as one call: y = irfft(rfft(s, n) * H)
template<typename T>
static inline tensor<T> filter_fft(const tensor<T> &s, const tensor<T> &H) noexcept { return dsc_filter_fft(ctx, s.x_, H.x_, nullptr); }

// Section D of dsc_mi355x.h: short-time transforms, frames-major spectrum [.., n_frames, n_fft/2 + 1] (complex payload, like rfft<T>);
// window = nullptr: ones.  pad_mode 0 = reflect, 1 = zeros; length <= 0: the natural length.
template<typename T>
static inline tensor<T> stft(const tensor<T> &x, int n_fft, int hop, const tensor<T> *window = nullptr, bool center = true, int pad_mode = 0) noexcept {
    return dsc_stft(ctx, x.x_, n_fft, hop, window ? window->x_ : nullptr, center, pad_mode, nullptr);
}
template<typename T>
static inline tensor<T> istft(const tensor<T> &X, int n_fft, int hop, const tensor<T> *window = nullptr, bool center = true, int length = -1) noexcept {
    return dsc_istft(ctx, X.x_, n_fft, hop, window ? window->x_ : nullptr, center, length, nullptr);
}

// Section E of dsc_mi355x.h: linear convolution of every row of x with one filter h; mode 0 = full, 1 = same, 2 = valid
// (numpy.convolve / numpy.correlate along the last axis).
template<typename T>
static inline tensor<T> convolve(const tensor<T> &x, const tensor<T> &h, int mode = 0) noexcept { return dsc_convolve(ctx, x.x_, h.x_, mode, nullptr); }
template<typename T>
static inline tensor<T> correlate(const tensor<T> &x, const tensor<T> &h, int mode = 2) noexcept { return dsc_correlate(ctx, x.x_, h.x_, mode, nullptr); }

// Section G of dsc_mi355x.h: analytic signal along the last axis (scipy.signal.hilbert(x, N) — complex payload, like rfft<T> — and its
// absolute value); n <= 0: the row length, rounded up to a power of two
template<typename T>
static inline tensor<T> hilbert(const tensor<T> &x, int n = -1) noexcept { return dsc_hilbert(ctx, x.x_, nullptr, n); }
template<typename T>
static inline tensor<T> envelope(const tensor<T> &x, int n = -1) noexcept { return dsc_envelope(ctx, x.x_, nullptr, n); }

// Section H of dsc_mi355x.h: polyphase FIR resampling along the last axis (scipy.signal.upfirdn / resample_poly / decimate with
// ftype='fir') and the low-pass window design; window 0 = hamming, 1 = kaiser
template<typename T>
static inline tensor<T> upfirdn(const tensor<T> &h, const tensor<T> &x, int up = 1, int down = 1) noexcept { return dsc_upfirdn(ctx, h.x_, x.x_, up, down, nullptr); }
template<typename T>
static inline tensor<T> resample_poly(const tensor<T> &x, int up, int down) noexcept { return dsc_resample_poly(ctx, x.x_, up, down, nullptr, nullptr); }
template<typename T>
static inline tensor<T> resample_poly(const tensor<T> &x, int up, int down, const tensor<T> &taps) noexcept { return dsc_resample_poly(ctx, x.x_, up, down, taps.x_, nullptr); }
template<typename T>
static inline tensor<T> decimate(const tensor<T> &x, int q, int n = 0) noexcept { return dsc_decimate(ctx, x.x_, q, n, nullptr); }
template<typename T>
static inline tensor<T> firwin(int numtaps, double cutoff, int window = 0, double beta = 5.0) noexcept { return dsc_firwin(ctx, numtaps, cutoff, window, beta, dtype_of<T>::value); }

// Section I of dsc_mi355x.h: prefix scans along one axis (numpy.cumsum / diff / unwrap) and phase(z) = unwrap(angle(z)) in one pass
// (a complex payload in, a real one out)
template<typename T>
static inline tensor<T> cumsum(const tensor<T> &x, int axis = -1) noexcept { return dsc_cumsum(ctx, x.x_, nullptr, axis); }
template<typename T>
static inline tensor<T> diff(const tensor<T> &x, int axis = -1) noexcept { return dsc_diff(ctx, x.x_, nullptr, axis); }
template<typename T>
static inline tensor<T> unwrap(const tensor<T> &x, int axis = -1) noexcept { return dsc_unwrap(ctx, x.x_, nullptr, axis); }
template<typename T>
static inline tensor<T> phase(const tensor<T> &z, int axis = -1) noexcept { return dsc_phase(ctx, z.x_, nullptr, axis); }

// Section J of dsc_mi355x.h: index maps along axes (numpy.roll / flip / fft.fftshift / fft.ifftshift / pad), bit-identical to numpy.
// roll(x, shift) rolls the flattened tensor, roll(x, shift, axis) one axis, roll(x, {shifts}, {axes}) several; flip / fftshift /
// ifftshift(x) take every axis, (x, {axes}) the listed ones; pad(x, {before, after, ...}, mode, value): one pair per axis of x, mode
// 0 constant, 1 edge, 2 reflect, 3 symmetric, 4 wrap, the constant as (re, im)
template<typename T>
static inline tensor<T> roll(const tensor<T> &x, int shift) noexcept { return dsc_roll(ctx, x.x_, nullptr, 0, &shift, nullptr); }
template<typename T>
static inline tensor<T> roll(const tensor<T> &x, int shift, int axis) noexcept { return dsc_roll(ctx, x.x_, nullptr, 1, &shift, &axis); }
template<typename T>
static inline tensor<T> roll(const tensor<T> &x, std::initializer_list<int> shifts, std::initializer_list<int> axes) noexcept {
    const std::vector<int> s(shifts), a(axes);
    return dsc_roll(ctx, x.x_, nullptr, (int) (s.size() < a.size() ? s.size() : a.size()), s.data(), a.data());
}
template<typename T>
static inline tensor<T> flip(const tensor<T> &x, std::initializer_list<int> axes = {}) noexcept {
    const std::vector<int> a(axes);
    return dsc_flip(ctx, x.x_, nullptr, (int) a.size(), a.data());
}
template<typename T>
static inline tensor<T> fftshift(const tensor<T> &x, std::initializer_list<int> axes = {}) noexcept {
    const std::vector<int> a(axes);
    return dsc_fftshift(ctx, x.x_, nullptr, (int) a.size(), a.data());
}
template<typename T>
static inline tensor<T> ifftshift(const tensor<T> &x, std::initializer_list<int> axes = {}) noexcept {
    const std::vector<int> a(axes);
    return dsc_ifftshift(ctx, x.x_, nullptr, (int) a.size(), a.data());
}
template<typename T>
static inline tensor<T> pad(const tensor<T> &x, std::initializer_list<int> pad_width, int mode = 0, double value_re = 0, double value_im = 0) noexcept {
    std::vector<int> w(pad_width);
    w.resize(2 * (size_t) x.ndim(), 0);
    return dsc_pad(ctx, x.x_, nullptr, w.data(), mode, value_re, value_im);
}

// Section K of dsc_mi355x.h: moments along one axis, every sum in double.  sumsq / rms / var / std of a complex payload carry a real
// one (as phase does); vdot(a, b) = sum conj(a) b; detrend takes out the mean (DSC_DETREND_CONSTANT) or the least-squares line
template<typename T>
static inline tensor<T> sumsq(const tensor<T> &x, int axis = -1, bool keep_dims = true) noexcept { return dsc_sumsq(ctx, x.x_, nullptr, axis, keep_dims); }
template<typename T>
static inline tensor<T> rms(const tensor<T> &x, int axis = -1, bool keep_dims = true) noexcept { return dsc_rms(ctx, x.x_, nullptr, axis, keep_dims); }
template<typename T>
static inline tensor<T> var(const tensor<T> &x, int axis = -1, int ddof = 0, bool keep_dims = true) noexcept { return dsc_var(ctx, x.x_, nullptr, axis, ddof, keep_dims); }
template<typename T>
static inline tensor<T> std(const tensor<T> &x, int axis = -1, int ddof = 0, bool keep_dims = true) noexcept { return dsc_std(ctx, x.x_, nullptr, axis, ddof, keep_dims); }
template<typename T>
static inline tensor<T> vdot(const tensor<T> &a, const tensor<T> &b, int axis = -1, bool keep_dims = true) noexcept { return dsc_vdot(ctx, a.x_, b.x_, nullptr, axis, keep_dims); }
template<typename T>
static inline tensor<T> detrend(const tensor<T> &x, int axis = -1, dsc_detrend_type type = DSC_DETREND_LINEAR) noexcept { return dsc_detrend(ctx, x.x_, nullptr, axis, type); }

static inline void synchronize() noexcept { dsc_synchronize(ctx); }

}  // namespace dsc
