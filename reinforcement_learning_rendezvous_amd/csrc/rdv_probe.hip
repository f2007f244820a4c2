// rdv_probe.hip — test infrastructure, never part of the product: librdv_probe.so.
//
// Each numerical primitive of rdv_device.h behind a trivial element-wise kernel and a C entry point, so that tests/test_gpu_device_math.py
// can pin it to a 50-digit reference on its own (the transition tests compare whole steps at 1e-10 .. 1e-6: a primitive could be 1e-12
// off underneath them).  Compiled with exactly the HIPFLAGS of the product (csrc/Makefile): the same contraction, the same optimiser.
// librdv_hip.so gains no symbol from this file; nothing of the product links or loads it.
//
// Every entry point: device pointers in and out (never aliased), n elements, a stream; one thread per element, 256-thread blocks, a
// ragged last block.  Vectors are rows of a dense row-major array (n x 3, n x 4, n x 7, n x 9).  Returns 0, -1 for a negative n or
// -3 for a launch error.
#include "rdv_device.h"

#include <cmath>

using namespace rdv;

namespace {

constexpr int kProbeBlock = 256;

template <typename F>
__global__ void __launch_bounds__(kProbeBlock) each_kernel(int64_t n, F f) {
  const int64_t i = (int64_t)blockIdx.x * kProbeBlock + threadIdx.x;
  if (i < n) f(i);
}

template <typename F>
int each(int64_t n, hipStream_t stream, F f) {
  if (n < 0 || n > ((int64_t)1 << 31)) return -1;
  if (n == 0) return 0;
  each_kernel<<<dim3((unsigned)((n + kProbeBlock - 1) / kProbeBlock)), dim3(kProbeBlock), 0, stream>>>(n, f);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

enum : int { SERIES_TINY = 0, SERIES_SMALL = 1, SERIES_LARGE = 2, SERIES_DISPATCH = 3 };

template <int kSeries>
int cos_sinc_probe(const double* u, double* c, double* sc, int64_t n, hipStream_t stream) {
  return each(n, stream, [=] __device__(int64_t i) {
    double cv, sv;
    if (kSeries == SERIES_TINY) cos_sinc_tiny(u[i], cv, sv);
    else if (kSeries == SERIES_SMALL) cos_sinc_small(u[i], cv, sv);
    else if (kSeries == SERIES_LARGE) cos_sinc_large(u[i], cv, sv);
    else cos_sinc(u[i], cv, sv);
    c[i] = cv; sc[i] = sv;
  });
}

template <bool kRaw>
int integrate_attitude_probe(const double* q, const double* w, double half_dt, double* out, int64_t n, hipStream_t stream) {
  return each(n, stream, [=] __device__(int64_t i) {
    double qv[4] = {q[4 * i], q[4 * i + 1], q[4 * i + 2], q[4 * i + 3]};
    const double wv[3] = {w[3 * i], w[3 * i + 1], w[3 * i + 2]};
    integrate_attitude<kRaw>(qv, wv, half_dt);
    for (int j = 0; j < 4; ++j) out[4 * i + j] = qv[j];
  });
}

}  // namespace

extern "C" {

int rdvprobe_rsqrt64(const double* x, double* y, int64_t n, hipStream_t stream) {
  return each(n, stream, [=] __device__(int64_t i) { y[i] = rsqrt64(x[i]); });
}

int rdvprobe_cos_sinc_tiny(const double* u, double* c, double* sc, int64_t n, hipStream_t stream) { return cos_sinc_probe<SERIES_TINY>(u, c, sc, n, stream); }
int rdvprobe_cos_sinc_small(const double* u, double* c, double* sc, int64_t n, hipStream_t stream) { return cos_sinc_probe<SERIES_SMALL>(u, c, sc, n, stream); }
int rdvprobe_cos_sinc_large(const double* u, double* c, double* sc, int64_t n, hipStream_t stream) { return cos_sinc_probe<SERIES_LARGE>(u, c, sc, n, stream); }
int rdvprobe_cos_sinc(const double* u, double* c, double* sc, int64_t n, hipStream_t stream) { return cos_sinc_probe<SERIES_DISPATCH>(u, c, sc, n, stream); }

int rdvprobe_pow_minus_fifth(const double* x, double* y, int64_t n, hipStream_t stream) {
  return each(n, stream, [=] __device__(int64_t i) { y[i] = pow_minus_fifth(x[i]); });
}

int rdvprobe_div_1e5(const double* k, double* y, int64_t n, hipStream_t stream) {
  return each(n, stream, [=] __device__(int64_t i) { y[i] = div_1e5(k[i]); });
}

// The table of attitude_error_of as the host fills it for a handle (rdv_create in rdv_hip.hip: the same expression, this host's libm;
// a change there is made here too: the comment at that line says so):
// `host_table` takes 200,001 doubles, acos(k / 1e5) for k = -100000 .. 100000.  Host memory; no device is touched.
int rdvprobe_fill_acos_table(double* host_table) {
  if (!host_table) return -1;
  for (int k = 0; k < 200001; ++k) host_table[k] = std::acos((double)(k - 100000) / 1e5);
  return 0;
}
// `table`: the 200,001 doubles above, in device memory
int rdvprobe_attitude_error_of(const double* table, const double* k, double* y, int64_t n, hipStream_t stream) {
  return each(n, stream, [=] __device__(int64_t i) {
    DevParams P = {};
    P.acos_table = table;
    y[i] = attitude_error_of(P, k[i]);
  });
}

// lo, span, inv_span are wave-uniform, as the three triples of the parameter block are
int rdvprobe_normalized(const double* val, double lo, double span, double inv_span, float* y, int64_t n, hipStream_t stream) {
  return each(n, stream, [=] __device__(int64_t i) { y[i] = normalized(val[i], lo, span, inv_span); });
}

int rdvprobe_u21(const uint32_t* field, double* y, int64_t n, hipStream_t stream) {
  return each(n, stream, [=] __device__(int64_t i) { y[i] = u21(field[i]); });
}
int rdvprobe_s21(const uint32_t* field, double* y, int64_t n, hipStream_t stream) {
  return each(n, stream, [=] __device__(int64_t i) { y[i] = s21(field[i]); });
}

// counter: n x 4 words, key: n x 2 words, out: n x 4 words
int rdvprobe_philox4x32_10(const uint32_t* counter, const uint32_t* key, uint32_t* out, int64_t n, hipStream_t stream) {
  return each(n, stream, [=] __device__(int64_t i) {
    uint32_t c0 = counter[4 * i], c1 = counter[4 * i + 1], c2 = counter[4 * i + 2], c3 = counter[4 * i + 3];
    philox4x32_10(c0, c1, c2, c3, key[2 * i], key[2 * i + 1]);
    out[4 * i] = c0; out[4 * i + 1] = c1; out[4 * i + 2] = c2; out[4 * i + 3] = c3;
  });
}

int rdvprobe_unit_vector(const double* v, double* out, int64_t n, hipStream_t stream) {
  return each(n, stream, [=] __device__(int64_t i) {
    double o[3];
    unit_vector(v[3 * i], v[3 * i + 1], v[3 * i + 2], o);
    for (int j = 0; j < 3; ++j) out[3 * i + j] = o[j];
  });
}

// axis: n x 3 (unit), theta: n, nominal: n x 4 (unit), tiny: the wave-uniform flag the parameters set (qc0_tiny / qt0_tiny); out: n x 4
int rdvprobe_deviate(const double* axis, const double* theta, const double* nominal, int tiny, double* out, int64_t n, hipStream_t stream) {
  const bool is_tiny = tiny != 0;
  return each(n, stream, [=] __device__(int64_t i) {
    const double a[3] = {axis[3 * i], axis[3 * i + 1], axis[3 * i + 2]};
    const double b[4] = {nominal[4 * i], nominal[4 * i + 1], nominal[4 * i + 2], nominal[4 * i + 3]};
    double o[4];
    deviate(a, theta[i], b, is_tiny, o);
    for (int j = 0; j < 4; ++j) out[4 * i + j] = o[j];
  });
}

int rdvprobe_quat2mat(const double* q, double* m, int64_t n, hipStream_t stream) {
  return each(n, stream, [=] __device__(int64_t i) {
    const double qv[4] = {q[4 * i], q[4 * i + 1], q[4 * i + 2], q[4 * i + 3]};
    double mv[9];
    quat2mat(qv, mv);
    for (int j = 0; j < 9; ++j) m[9 * i + j] = mv[j];
  });
}

// raw != 0: integrate_attitude<true> (the first step after a state was injected), else integrate_attitude<false>
int rdvprobe_integrate_attitude(const double* q, const double* w, double half_dt, int raw, double* out, int64_t n, hipStream_t stream) {
  return raw ? integrate_attitude_probe<true>(q, w, half_dt, out, n, stream) : integrate_attitude_probe<false>(q, w, half_dt, out, n, stream);
}

int rdvprobe_rms7(const double* x, double* y, int64_t n, hipStream_t stream) {
  return each(n, stream, [=] __device__(int64_t i) {
    double xv[7];
    for (int j = 0; j < 7; ++j) xv[j] = x[7 * i + j];
    y[i] = rms7(xv);
  });
}

}  // extern "C"
