// FrodoKEM per-row calls: the host entry points of the internal interface (qrkem_internal.h) over the kernels and
// launchers of frodo_kernels.cuh, one switch per call on the parameter set and on how A is generated.
#include "frodo_kernels.cuh"

namespace qrk {
namespace frodo {

// Tests only (qrk_dbg_frodo_sample): the caller's 16-bit words, spec order [n][4 W], into the tiled stream the
// sponge kernels write (one thread per u64 = 4 words, little-endian as squeezed).
__global__ __launch_bounds__(256) void k_fr_dbg_tile(const uint16_t* __restrict__ words, size_t n, int W,
                                                     uint64_t* __restrict__ raw) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t hs = t / W;
  const int w = (int)(t % W);
  if (hs >= n) return;
  const uint16_t* p = words + t * 4;
  raw[tidx(hs, w, W)] = (uint64_t)p[0] | (uint64_t)p[1] << 16 | (uint64_t)p[2] << 32 | (uint64_t)p[3] << 48;
}

// The sampler alone on a chosen stream: the launch of encaps_t / keypair_t on the context's scratch, then its
// three regions (S' / S^T with the pad columns, E' / E, E'') copied out whole.
template <int N, bool KG>
hipError_t dbg_sample_t(size_t n, const uint16_t* words, int8_t* s8, int16_t* e16, int16_t* epp16, void* scratch,
                        hipStream_t st) {
  using P = FP<N>;
  constexpr int W = KG ? P::KG_WORDS : P::SE_WORDS;
  const View<N> v = carve<N>(scratch, round64(n));
  QRK_LAUNCH("k_fr_dbg_tile", st, k_fr_dbg_tile, dim3(blocks_for(n * W)), dim3(256), 0, st, words, n, W, v.raw);
  launch_sample<N, KG>(v, n, st);
  qrk_chk(hipMemcpyAsync(s8, v.sp8, n * NBAR * P::NP, hipMemcpyDeviceToDevice, st));
  qrk_chk(hipMemcpyAsync(e16, v.ep16, n * NBAR * N * 2, hipMemcpyDeviceToDevice, st));
  if (!KG) qrk_chk(hipMemcpyAsync(epp16, v.epp16, n * 64 * 2, hipMemcpyDeviceToDevice, st));
  return launch_status();
}

}  // namespace frodo

int frodo_sample_max(const AlgInfo& a) {
  switch (a.k) {
    case 640: return frodo::FP<640>::SMAX;
    case 976: return frodo::FP<976>::SMAX;
    case 1344: return frodo::FP<1344>::SMAX;
  }
  return 0;
}

size_t frodo_sample_pitch(const AlgInfo& a) {
  switch (a.k) {
    case 640: return frodo::FP<640>::NP;
    case 976: return frodo::FP<976>::NP;
    case 1344: return frodo::FP<1344>::NP;
  }
  return 0;
}

hipError_t frodo_dbg_sample(const AlgInfo& a, bool kg, size_t n, const uint16_t* words, int8_t* s8, int16_t* e16,
                            int16_t* epp16, void* scratch, hipStream_t st) {
  if (n == 0) return hipSuccess;
  switch (a.k * 2 + (kg ? 1 : 0)) {
    case 1280: return frodo::dbg_sample_t<640, false>(n, words, s8, e16, epp16, scratch, st);
    case 1281: return frodo::dbg_sample_t<640, true>(n, words, s8, e16, epp16, scratch, st);
    case 1952: return frodo::dbg_sample_t<976, false>(n, words, s8, e16, epp16, scratch, st);
    case 1953: return frodo::dbg_sample_t<976, true>(n, words, s8, e16, epp16, scratch, st);
    case 2688: return frodo::dbg_sample_t<1344, false>(n, words, s8, e16, epp16, scratch, st);
    case 2689: return frodo::dbg_sample_t<1344, true>(n, words, s8, e16, epp16, scratch, st);
  }
  return hipErrorInvalidValue;
}

hipError_t frodo_dbg_from_samples(const AlgInfo& a, bool kg, size_t n, const int8_t* s8, const int16_t* e16,
                                  const int16_t* epp16, const uint8_t* in, const uint8_t* mu, uint8_t* out,
                                  uint8_t* sk, void* scratch, hipStream_t st) {
  if (n == 0) return hipSuccess;
  switch (a.k * 2 + (a.aes ? 1 : 0)) {
    case 1280: return frodo::dbg_from_samples_t<640, false>(kg, n, s8, e16, epp16, in, mu, out, sk, scratch, st);
    case 1281: return frodo::dbg_from_samples_t<640, true>(kg, n, s8, e16, epp16, in, mu, out, sk, scratch, st);
    case 1952: return frodo::dbg_from_samples_t<976, false>(kg, n, s8, e16, epp16, in, mu, out, sk, scratch, st);
    case 1953: return frodo::dbg_from_samples_t<976, true>(kg, n, s8, e16, epp16, in, mu, out, sk, scratch, st);
    case 2688: return frodo::dbg_from_samples_t<1344, false>(kg, n, s8, e16, epp16, in, mu, out, sk, scratch, st);
    case 2689: return frodo::dbg_from_samples_t<1344, true>(kg, n, s8, e16, epp16, in, mu, out, sk, scratch, st);
  }
  return hipErrorInvalidValue;
}

hipError_t frodo_trace_mu(const AlgInfo& a, size_t n, void* scratch, uint8_t* mu_out, hipStream_t st) {
  if (n == 0) return hipSuccess;
  switch (a.k) {
    case 640: return frodo::trace_mu_t<640>(n, scratch, mu_out, st);
    case 976: return frodo::trace_mu_t<976>(n, scratch, mu_out, st);
    case 1344: return frodo::trace_mu_t<1344>(n, scratch, mu_out, st);
  }
  return hipErrorInvalidValue;
}

hipError_t frodo_cleanse(const AlgInfo& a, size_t n, void* scratch, hipStream_t st) {
  if (n == 0) return hipSuccess;
  switch (a.k) {
    case 640: return frodo::cleanse_t<640>(n, scratch, st);
    case 976: return frodo::cleanse_t<976>(n, scratch, st);
    case 1344: return frodo::cleanse_t<1344>(n, scratch, st);
  }
  return hipErrorInvalidValue;
}

size_t frodo_scratch_bytes(const AlgInfo& a, size_t chunk) {
  const size_t C = round64(chunk);
  switch (a.k) {
    case 640: return frodo::scratch_bytes_t<640>(C);
    case 976: return frodo::scratch_bytes_t<976>(C);
    case 1344: return frodo::scratch_bytes_t<1344>(C);
  }
  return 0;
}

hipError_t frodo_keypair(const AlgInfo& a, size_t n, uint8_t* pk, uint8_t* sk, const uint8_t* coins, void* scratch,
                         const Streams& s) {
  if (n == 0) return hipSuccess;
  switch (a.k * 2 + (a.aes ? 1 : 0)) {
    case 1280: return frodo::keypair_t<640, false>(n, pk, sk, coins, scratch, s.main);
    case 1281: return frodo::keypair_t<640, true>(n, pk, sk, coins, scratch, s.main);
    case 1952: return frodo::keypair_t<976, false>(n, pk, sk, coins, scratch, s.main);
    case 1953: return frodo::keypair_t<976, true>(n, pk, sk, coins, scratch, s.main);
    case 2688: return frodo::keypair_t<1344, false>(n, pk, sk, coins, scratch, s.main);
    case 2689: return frodo::keypair_t<1344, true>(n, pk, sk, coins, scratch, s.main);
  }
  return hipErrorInvalidValue;
}

hipError_t frodo_encaps(const AlgInfo& a, size_t n, uint8_t* ct, uint8_t* ss, const uint8_t* pk, const uint8_t* coins,
                        int32_t*, void* scratch, const Streams& s) {
  if (n == 0) return hipSuccess;
  switch (a.k * 2 + (a.aes ? 1 : 0)) {
    case 1280: return frodo::encaps_t<640, false>(n, ct, ss, pk, coins, scratch, s.main);
    case 1281: return frodo::encaps_t<640, true>(n, ct, ss, pk, coins, scratch, s.main);
    case 1952: return frodo::encaps_t<976, false>(n, ct, ss, pk, coins, scratch, s.main);
    case 1953: return frodo::encaps_t<976, true>(n, ct, ss, pk, coins, scratch, s.main);
    case 2688: return frodo::encaps_t<1344, false>(n, ct, ss, pk, coins, scratch, s.main);
    case 2689: return frodo::encaps_t<1344, true>(n, ct, ss, pk, coins, scratch, s.main);
  }
  return hipErrorInvalidValue;
}

hipError_t frodo_decaps(const AlgInfo& a, size_t n, uint8_t* ss, const uint8_t* ct, const uint8_t* sk, int32_t*,
                        void* scratch, const Streams& s) {
  if (n == 0) return hipSuccess;
  switch (a.k * 2 + (a.aes ? 1 : 0)) {
    case 1280: return frodo::decaps_t<640, false>(n, ss, ct, sk, scratch, s.main);
    case 1281: return frodo::decaps_t<640, true>(n, ss, ct, sk, scratch, s.main);
    case 1952: return frodo::decaps_t<976, false>(n, ss, ct, sk, scratch, s.main);
    case 1953: return frodo::decaps_t<976, true>(n, ss, ct, sk, scratch, s.main);
    case 2688: return frodo::decaps_t<1344, false>(n, ss, ct, sk, scratch, s.main);
    case 2689: return frodo::decaps_t<1344, true>(n, ss, ct, sk, scratch, s.main);
  }
  return hipErrorInvalidValue;
}

}  // namespace qrk
