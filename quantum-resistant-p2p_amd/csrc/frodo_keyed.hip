// FrodoKEM key sets: the host entry points of the internal interface (qrkem_internal.h) over the kernels and launchers
// of frodo_keyed.cuh, where the design is described.
#include "frodo_keyed.cuh"

namespace qrk {

int frodo_keyed_tile_rows() { return frodo::FRK_TH; }

size_t frodo_keyset_bytes(const AlgInfo& a, bool secret, size_t g) {
  return frodo::set_layout((size_t)a.k, secret, g).total;
}

FrodoKeys frodo_keyset_view(const AlgInfo& a, bool secret, size_t g, void* mem) {
  return frodo::view_of((size_t)a.k, secret, g, mem);
}

hipError_t frodo_keyset_expand(const AlgInfo& a, bool secret, size_t g, const uint8_t* keys, void* mem,
                               hipStream_t st) {
  return frodo::with_n(a, [&](auto n_) {
    return frodo::expand_t<decltype(n_)::value>(a.aes, secret, g, keys, nullptr, mem, st);
  });
}

size_t frodo_keyed_scratch_bytes(const AlgInfo& a, size_t chunk, size_t g) {
  const size_t C = round64(chunk);
  switch (a.k) {
    case 640: return frodo::keyed_scratch_t<640>(C, g);
    case 976: return frodo::keyed_scratch_t<976>(C, g);
    case 1344: return frodo::keyed_scratch_t<1344>(C, g);
  }
  return 0;
}

hipError_t frodo_keyed_cleanse(const AlgInfo& a, size_t n, size_t g, void* scratch, hipStream_t st) {
  if (n == 0) return hipSuccess;
  const size_t C = round64(n);
  return frodo::with_n(a, [&](auto n_) {
    const auto v = frodo::keyed_carve<decltype(n_)::value>(scratch, C, g);
    return hipMemsetAsync(v.seeds, 0, (size_t)((uint8_t*)v.perm - (uint8_t*)v.seeds), st);  // seeds | kk
  });
}

hipError_t frodo_encaps_keyed(const AlgInfo& a, const FrodoKeys& ks, size_t n, const uint32_t* key_index, uint8_t* ct,
                              uint8_t* ss, const uint8_t* coins, int32_t* status, void* scratch, const Streams& s) {
  if (n == 0) return hipSuccess;
  return frodo::with_n(a, [&](auto n_) {
    return frodo::encaps_keyed_t<decltype(n_)::value>(ks, n, key_index, ct, ss, coins, status, scratch, s.main);
  });
}

hipError_t frodo_decaps_keyed(const AlgInfo& a, const FrodoKeys& ks, size_t n, const uint32_t* key_index, uint8_t* ss,
                              const uint8_t* ct, int32_t* status, void* scratch, const Streams& s) {
  if (n == 0) return hipSuccess;
  return frodo::with_n(a, [&](auto n_) {
    return frodo::decaps_keyed_t<decltype(n_)::value>(ks, n, key_index, ss, ct, status, scratch, s.main);
  });
}

}  // namespace qrk
