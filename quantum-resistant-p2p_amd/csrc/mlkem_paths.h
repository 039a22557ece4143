// ML-KEM: the host entry of every execution path, as the dispatch in mlkem.hip calls them.  Each is
// defined in its path's own file (all of them compiled as part of mlkem.hip), which instantiates that
// path's kernels for the module rank
// k = 2, 3, 4 (any other k: hipErrorInvalidValue).  n > 0 handshakes, one chunk.
#pragma once
#include "qrkem_internal.h"

namespace qrk {
namespace mlkem {

// f(std::integral_constant<int, K>{}) for K = k
template <class F>
inline hipError_t with_rank(int k, F&& f) {
  switch (k) {
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
  }
  return hipErrorInvalidValue;
}

// mlkem_batch.cuh: the multi-role schedule
hipError_t keygen_batched(int k, size_t n, uint8_t* pk, uint8_t* sk, const uint8_t* coins, void* scratch,
                          const Streams& s);
hipError_t encaps_batched(int k, size_t n, uint8_t* ct, uint8_t* ss, const uint8_t* pk, const uint8_t* coins,
                          int32_t* status, void* scratch, const Streams& s);
hipError_t decaps_batched(int k, size_t n, uint8_t* ss, const uint8_t* ct, const uint8_t* sk, void* scratch,
                          const Streams& s);

// mlkem_one.cuh: one launch per operation, n <= mlkem_small_max()
hipError_t keygen_one(int k, size_t n, uint8_t* pk, uint8_t* sk, const uint8_t* coins, const Streams& s);
hipError_t encaps_one(int k, size_t n, uint8_t* ct, uint8_t* ss, const uint8_t* pk, const uint8_t* coins,
                      int32_t* status, const Streams& s);
hipError_t decaps_one(int k, size_t n, uint8_t* ss, const uint8_t* ct, const uint8_t* sk, const Streams& s);

// mlkem_kg.cuh: the single-shot multi-workgroup KeyGens, n <= mlkem_kg_multi_max()
bool keygen_pipe_built();                // QRK_KG_PIPE
size_t keygen_scratch_bytes(size_t n);   // what they keep at the start of the scratch for n handshakes
hipError_t keygen_pipe(int k, size_t n, uint8_t* pk, uint8_t* sk, const uint8_t* coins, void* scratch,
                       const Streams& s);
hipError_t keygen_multi(int k, size_t n, uint8_t* pk, uint8_t* sk, const uint8_t* coins, void* scratch,
                        const Streams& s);

}  // namespace mlkem
}  // namespace qrk
