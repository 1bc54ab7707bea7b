// inverse.hpp -- header-only C++ adapter of the device inverse-or-zero (inverse.h) on the types of ring.hpp.
// Beside ring.hpp for the reason given in r1cs_check.h; it includes ring.hpp, so one include gives both.
#ifndef RINGSNARK_AMD_INVERSE_HPP
#define RINGSNARK_AMD_INVERSE_HPP

#include "inverse.h"
#include "ring.hpp"

namespace ringsnark::amd {

// The device-resident form: element e of x is the ring element at x_row + e * x_stride ring elements of x_buf, likewise
// num (num_buf == nullptr: no numerator) and out.  The buffers may be one assignment (blocks x, inv, z or a, b, binv, y) as
// long as no x or num row is an output row; num may be x.  report == nullptr: enqueued only.  Returns true when no word is
// bad (inverse.h says what bad means; zeros are ordinary input); always true without a report.
inline bool inv_or_zero(const DeviceWords &x_buf, size_t x_row, size_t x_stride, const DeviceWords *num_buf, size_t num_row, size_t num_stride,
                        size_t count, DeviceWords &out_buf, size_t out_row, size_t out_stride, rs_inv_report *report = nullptr) {
  const size_t rw = Context::ring_words();
  if (count) {
    if (x_stride < 1 || x_row + (count - 1) * x_stride + 1 > x_buf.words() / rw)
      throw std::invalid_argument("inv_or_zero: the input rows do not fit their buffer");
    if (num_buf && (num_stride < 1 || num_row + (count - 1) * num_stride + 1 > num_buf->words() / rw))
      throw std::invalid_argument("inv_or_zero: the numerator rows do not fit their buffer");
    if (out_stride < 1 || out_row + (count - 1) * out_stride + 1 > out_buf.words() / rw)
      throw std::invalid_argument("inv_or_zero: the output rows do not fit their buffer");
  }
  check(rs_ring_inv_or_zero(Context::get_context(), x_buf.get() + x_row * rw, x_stride, num_buf ? num_buf->get() + num_row * rw : nullptr,
                            num_stride, count, out_buf.get() + out_row * rw, out_stride, report, nullptr));
  return !report || report->n_bad == 0;
}

// The value forms: the ring element whose slots hold x^-1 where x's slot is non-zero and 0 where it is zero (the witness of
// the is-zero gadget), and num * x^-1 likewise (a quotient wire).  *report says where x is zero.
inline RingElem inv_or_zero(const RingElem &x, const RingElem &num, rs_inv_report *report = nullptr) {
  const size_t rw = Context::ring_words();
  const RingElem xp = x.to_poly(), np = num.to_poly();
  const DeviceWords dx(xp.get_poly().data(), rw), dn(np.get_poly().data(), rw);
  DeviceWords dout(rw);
  rs_inv_report rep;
  inv_or_zero(dx, 0, 1, &dn, 0, 1, 1, dout, 0, 1, &rep);
  if (report) *report = rep;
  std::vector<uint64_t> h(rw);
  dout.download(h.data());
  return RingElem(std::move(h));
}
inline RingElem inv_or_zero(const RingElem &x, rs_inv_report *report = nullptr) {
  const size_t rw = Context::ring_words();
  const RingElem xp = x.to_poly();
  const DeviceWords dx(xp.get_poly().data(), rw);
  DeviceWords dout(rw);
  rs_inv_report rep;
  inv_or_zero(dx, 0, 1, nullptr, 0, 1, 1, dout, 0, 1, &rep);
  if (report) *report = rep;
  std::vector<uint64_t> h(rw);
  dout.download(h.data());
  return RingElem(std::move(h));
}

}  // namespace ringsnark::amd
#endif
