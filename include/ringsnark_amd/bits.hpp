// bits.hpp -- header-only C++ adapter of the device bit decomposition (bits.h) on the types of ring.hpp.
// Beside ring.hpp for the reason given in r1cs_check.h; it includes ring.hpp, so one include gives both.
#ifndef RINGSNARK_AMD_BITS_HPP
#define RINGSNARK_AMD_BITS_HPP

#include "bits.h"
#include "ring.hpp"

namespace ringsnark::amd {

// The device-resident form: element e is the ring element at x + e * x_stride ring elements, its bit k goes to the ring
// element at bits + (e * bits_stride + k); both are word offsets into device buffers (x_buf and bits_buf may be the same
// buffer -- an assignment whose blocks are b_0 .. b_{nbits-1}, x -- as long as no x row is a bit row).  report == nullptr:
// enqueued only.  Returns true when no position is bad (bits.h says what bad means); always true without a report.
inline bool bit_decompose(const DeviceWords &x_buf, size_t x_row, size_t x_stride, size_t count, int nbits, DeviceWords &bits_buf,
                          size_t bits_row, size_t bits_stride, rs_bits_report *report = nullptr) {
  const size_t rw = Context::ring_words();
  if (count) {
    if (x_stride < 1 || x_row + (count - 1) * x_stride + 1 > x_buf.words() / rw)
      throw std::invalid_argument("bit_decompose: the input rows do not fit their buffer");
    if (nbits < 1 || bits_stride < (size_t)nbits || bits_row + (count - 1) * bits_stride + (size_t)nbits > bits_buf.words() / rw)
      throw std::invalid_argument("bit_decompose: the bit rows do not fit their buffer");
  }
  check(rs_ring_bit_decompose(Context::get_context(), x_buf.get() + x_row * rw, x_stride, count, nbits, bits_buf.get() + bits_row * rw,
                              bits_stride, report, nullptr));
  return !report || report->n_bad == 0;
}

// What pb_variable_array::fill_with_bits_of_field_element (gadgetlib/pb_variable.tcc:58-66, an empty stub in the reference)
// would have to do for a ring element: the nbits ring elements whose slots hold bit k of x's slot (the same in every limb;
// x must hold one integer below 2^nbits per slot, the same word in every limb -- *report says where it does not).
inline std::vector<RingElem> bit_decompose(const RingElem &x, int nbits, rs_bits_report *report = nullptr) {
  const size_t rw = Context::ring_words();
  const RingElem xp = x.to_poly();
  const DeviceWords dx(xp.get_poly().data(), rw);
  DeviceWords dbits((size_t)std::max(nbits, 1) * rw);
  rs_bits_report rep;
  bit_decompose(dx, 0, 1, 1, nbits, dbits, 0, (size_t)std::max(nbits, 1), &rep);
  if (report) *report = rep;
  std::vector<uint64_t> h(dbits.words());
  dbits.download(h.data());
  std::vector<RingElem> out;
  out.reserve((size_t)nbits);
  for (int k = 0; k < nbits; k++) out.emplace_back(std::vector<uint64_t>(h.begin() + (size_t)k * rw, h.begin() + (size_t)(k + 1) * rw));
  return out;
}

}  // namespace ringsnark::amd
#endif
