// inverse_run.cpp -- run-time check of ringsnark::amd::inv_or_zero (include/ringsnark_amd/inverse.hpp) against librs_hip.so:
// plain C++17, no HIP headers.  TEST INFRASTRUCTURE.
//
// usage: inverse_run N L q_0..q_{L-1} N_enc K Q_0..Q_{K-1}
// The is-zero assignment (row 0 the public wire `one`, then per block x, inv, z) of three elements with planted zeros: `one`,
// the x rows and the z rows are uploaded, the inv rows are made on the device inside the assignment, and x * inv = one - z
// and x * z = 0 hold under the adapter's own ring operations.  The value forms give the same rows, and a quotient times
// its divisor gives the numerator back.  Prints "inverse_run: OK blocks=B n_zero=Z first=E/L/S": the zeros the
// device reported (equal to those planted) and the first of them as element / limb / slot.
#include <cstdio>
#include <cstdlib>

#include <ringsnark_amd/inverse.hpp>

using namespace ringsnark::amd;

static int fails = 0;
#define EXPECT(c)                                         \
  do {                                                    \
    if (!(c)) {                                           \
      std::fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      fails++;                                            \
    }                                                     \
  } while (0)

static void run(int argc, char **argv, unsigned long long *line) {
  int a = 1;
  Params p;
  p.N = std::atoi(argv[a++]);
  p.L = std::atoi(argv[a++]);
  for (int i = 0; i < p.L; i++) p.q.push_back(std::strtoull(argv[a++], nullptr, 10));
  p.N_enc = std::atoi(argv[a++]);
  p.K = std::atoi(argv[a++]);
  for (int i = 0; i < p.K; i++) p.Q.push_back(std::strtoull(argv[a++], nullptr, 10));
  EXPECT(a == argc);
  Context::set_context(p);

  const size_t count = 3, n_vars = 1 + 3 * count, rw = Context::ring_words();
  std::vector<uint64_t> h(n_vars * rw, 0xDEADull);
  for (size_t i = 0; i < rw; i++) h[i] = 1;
  size_t planted = 0, first_key = ~(size_t)0;
  for (size_t blk = 0; blk < count; blk++) {
    const std::vector<uint64_t> x = RingElem::random_nonzero_element().get_poly();
    for (size_t i = 0; i < rw; i++) {
      // block 0 has no zero in limb 0; block 1 a zero in every fourth word; block 2 in every fifth
      const bool zero = x[i] == 0 || (blk == 0 ? i >= (size_t)p.N && i % 3 == 0 : i % (3 + blk) == 0);
      h[(1 + 3 * blk) * rw + i] = zero ? 0 : x[i];
      h[(3 + 3 * blk) * rw + i] = zero ? 1 : 0;
      if (zero) {
        planted++;
        if (first_key == ~(size_t)0) first_key = blk * rw + i;
      }
    }
  }
  DeviceWords asg(h.data(), h.size());
  rs_inv_report rep;
  EXPECT(inv_or_zero(asg, 1, 3, nullptr, 0, 1, count, asg, 2, 3, &rep));
  EXPECT(rep.n_bad == 0 && rep.bad_elem == 0 && rep.bad_limb == 0 && rep.bad_slot == 0 && rep.bad_x == 0 && rep.bad_num == 0);
  EXPECT(rep.n_zero == planted);
  EXPECT(planted == 0 || rep.zero_elem * rw + (size_t)rep.zero_limb * p.N + rep.zero_slot == first_key);
  std::vector<uint64_t> full(h.size());
  asg.download(full.data());
  for (size_t v = 0; v < n_vars; v++)
    if (v == 0 || (v - 1) % 3 != 1)
      for (size_t i = 0; i < rw; i++) EXPECT(full[v * rw + i] == h[v * rw + i]);  // every row but the inv rows is as it was

  std::vector<RingElem> wires;
  for (size_t v = 0; v < n_vars; v++) wires.emplace_back(std::vector<uint64_t>(full.begin() + v * rw, full.begin() + (v + 1) * rw));
  for (size_t blk = 0; blk < count; blk++) {
    const RingElem &x = wires[1 + 3 * blk], &inv = wires[2 + 3 * blk], &z = wires[3 + 3 * blk];
    EXPECT(x * inv == wires[0] - z);
    EXPECT((x * z).is_zero());
    rs_inv_report one_rep;
    EXPECT(inv_or_zero(x, &one_rep).get_poly() == inv.get_poly());  // the value form gives the same row
    EXPECT(one_rep.n_bad == 0);
    EXPECT(inv_or_zero(x, x, &one_rep) == wires[0] - z);  // num = x: the non-zero indicator
  }

  {  // a quotient: y * b = a for an invertible b, and y = a * b^-1 as rs_ring_inv has it
    const RingElem b = RingElem::random_invertible_element(), num = RingElem::random_element();
    const RingElem y = inv_or_zero(b, num, &rep);
    EXPECT(rep.n_zero == 0 && rep.n_bad == 0);
    EXPECT(y * b == num);
    EXPECT(y == num * b.inverse());
    EXPECT(inv_or_zero(b).get_poly() == b.inverse().get_poly());
  }

  {  // a word equal to q_0 in limb 0 is reported and gives 0
    std::vector<uint64_t> w = wires[1].get_poly();
    w[2] = p.q[0];
    const DeviceWords dx(w.data(), rw);
    DeviceWords dout(rw);
    EXPECT(!inv_or_zero(dx, 0, 1, nullptr, 0, 1, 1, dout, 0, 1, &rep));
    EXPECT(rep.n_bad == 1 && rep.bad_elem == 0 && rep.bad_limb == 0 && rep.bad_slot == 2 && rep.bad_x == p.q[0] && rep.bad_num == 0);
    std::vector<uint64_t> o(rw);
    dout.download(o.data());
    EXPECT(o[2] == 0);
  }

  try {  // an x row that is an output row
    inv_or_zero(asg, 1, 3, nullptr, 0, 1, count, asg, 1, 3, &rep);
    EXPECT(false);
  } catch (const std::exception &) {
  }
  try {  // rows past the end of the buffer
    inv_or_zero(asg, 1, 3, nullptr, 0, 1, count + 1, asg, 2, 3, &rep);
    EXPECT(false);
  } catch (const std::invalid_argument &) {
  }
  line[0] = count;
  line[1] = planted;
  line[2] = first_key / rw;
  line[3] = first_key % rw / (size_t)p.N;
  line[4] = first_key % (size_t)p.N;
}

int main(int argc, char **argv) {
  unsigned long long line[5] = {0, 0, 0, 0, 0};
  try {
    run(argc, argv, line);
  } catch (const std::exception &e) {  // reported as a failure, not as an abort
    std::fprintf(stderr, "FAIL exception: %s\n", e.what());
    fails++;
  }
  if (fails) {
    std::fprintf(stderr, "inverse_run: %d failure(s)\n", fails);
    return 1;
  }
  std::printf("inverse_run: OK blocks=%llu n_zero=%llu first=%llu/%llu/%llu\n", line[0], line[1], line[2], line[3], line[4]);
  return 0;
}
