// Test-only probe of the FrodoKEM key-set kernels (csrc/frodo_keyed.cuh), its own shared object built by
// csrc/Makefile with the library's flags, never linked into libqrkem.so; tests/test_gpu_frodo_keyed.py drives it.
// Hash-derived entries of A never reach the edges of the limb split (0x007F / 0x0080, 0x7F80 / 0x8000, 0xFF80), a
// generated A cannot be one-hot, and hash-derived samples never fill a tile: here A is the caller's matrix and S',
// E', E'' are the caller's, and the header's own launchers run on them -- the set's expansion with the matrix in
// place of Gen(A) (k_frk_split, k_frk_unpack), then the launches of the keyed Encaps after the sampler
// (k_frk_group, k_frk_sa, k_frk_pack).  Nothing of the header is written again here.
#include <hip/hip_runtime.h>

#include <vector>

#include "frodo_keyed.cuh"

// the launch-error channel and timer hook of QRK_LAUNCH, which libqrkem.so defines for itself
namespace qrk {
thread_local KernelTimer* g_timer = nullptr;
thread_local hipError_t g_launch_err = hipSuccess;
std::atomic<int> g_dbg_fail_launch{0};
}  // namespace qrk

using namespace qrk;
using namespace qrk::frodo;

// Every value of a device array of rows x pitch samples within [-max, max], and zero past the `used` leading columns
// of a row?  The kernels' accumulator bounds and the zero pad of S' hold for the sampler's output only.
template <class T>
static int in_range(const T* dev, size_t rows, size_t pitch, size_t used, int max) {
  std::vector<T> h(rows * pitch);
  if (hipMemcpy(h.data(), dev, rows * pitch * sizeof(T), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  for (size_t r = 0; r < rows; ++r)
    for (size_t c = 0; c < pitch; ++c) {
      const int v = h[r * pitch + c];
      if (c < used ? (v < -max || v > max) : v != 0) return 0;
    }
  return 1;
}

template <int N>
static int encrypt_t(size_t g, const uint8_t* pk, const uint16_t* matrix, size_t n, const uint32_t* key_index,
                     const int8_t* s8, const int16_t* e16, const int16_t* epp16, const uint8_t* mu, uint8_t* ct,
                     int fill) {
  using P = FP<N>;
  const int ok = in_range(s8, n * NBAR, (size_t)P::NP, (size_t)N, P::SMAX) > 0 &&
                 in_range(e16, n, (size_t)NBAR * N, (size_t)NBAR * N, P::SMAX) > 0 &&
                 in_range(epp16, n, (size_t)64, (size_t)64, P::SMAX) > 0;
  if (!ok) return -2;  // refused before any launch
  const SetLayout l = set_layout(N, false, g);
  const size_t scratch_bytes = keyed_scratch_t<N>(round64(n), g);
  void *mem = nullptr, *scratch = nullptr;
  hipError_t e = hipMalloc(&mem, l.total);
  if (e == hipSuccess) e = hipMalloc(&scratch, scratch_bytes);
  if (e == hipSuccess) e = hipMemset(scratch, fill, scratch_bytes);  // nothing below may rely on what it held
  if (e == hipSuccess) {
    launch_begin();
    e = expand_t<N>(false, false, g, pk, matrix, mem, nullptr);
  }
  if (e == hipSuccess) {
    e = dbg_keyed_from_samples_t<N>(view_of(N, false, g, mem), n, key_index, s8, e16, epp16, mu, ct, scratch, nullptr);
  }
  const hipError_t es = hipDeviceSynchronize();
  if (e == hipSuccess) e = es;
  (void)hipFree(scratch);
  (void)hipFree(mem);
  return (int)e;
}

extern "C" {

// ct [n][ct bytes] of n rows under a public set of g keys whose A is matrix, u16 [g][N][N] row-major, and whose B
// comes from pk [g][pk bytes]: row i uses key key_index[i] (a row with an index >= g gets a zero ct), S' = s8 int8
// [n][8][NP] (pad columns zero), E' = e16 int16 [n][8][N], E'' = epp16 int16 [n][64], mu [n][len_mu].  Every
// sample must lie in the sampler's range, |v| <= 12 / 10 / 6, and the pad columns of S' must be zero: the matrices
// are read back first and -2 is returned without a launch otherwise (the check of qrk_dbg_frodo_from_samples).
// Device pointers; set and scratch are allocated here, the scratch pre-filled with `fill`, and freed again.
// Returns the hipError_t, 0 for success.
int frk_probe_encrypt(int N, size_t g, const uint8_t* pk, const uint16_t* matrix, size_t n, const uint32_t* key_index,
                      const int8_t* s8, const int16_t* e16, const int16_t* epp16, const uint8_t* mu, uint8_t* ct,
                      int fill) {
  switch (N) {
    case 640: return encrypt_t<640>(g, pk, matrix, n, key_index, s8, e16, epp16, mu, ct, fill);
    case 976: return encrypt_t<976>(g, pk, matrix, n, key_index, s8, e16, epp16, mu, ct, fill);
    case 1344: return encrypt_t<1344>(g, pk, matrix, n, key_index, s8, e16, epp16, mu, ct, fill);
  }
  return (int)hipErrorInvalidValue;
}

int frk_probe_tile_rows(void) { return FRK_TH; }

}  // extern "C"
