// The launch routing of csrc/conv.hip, executed on the host: conv_route is a pure function of the launch parameters and the knobs (no HIP
// call, no static).  tests/test_conv_route.py cuts the text of `struct ConvParams` and of the routing section (ConvKnobs, ConvRoute,
// conv_route) out of conv.hip into conv_route_cut.inc; the SAME TEXT is compiled for x86 and compared with a Python restatement of the
// rules it replaced.  Test infrastructure: nothing here is linked into the product.
#include <cstdint>
namespace ssg {
#include "conv_route_cut.inc"
}
using namespace ssg;

extern "C" {
// q: n cases of 10 ints {M, Cout, Kpad, Cin, Cin2, residual?, second input?, epi, split, cin4}; knobs: the 7 fields of ConvKnobs in order;
// out: n x 6 ints {family, BM, BN, BK, dual, line}
void hx_conv_route(const int* q, long n, const int* knobs, int* out) {
  static float dummy;
  ConvKnobs k;
  k.dma = knobs[0]; k.line = knobs[1]; k.wide_mintiles = knobs[2]; k.bn64_maxtiles = knobs[3]; k.tall_mintiles = knobs[4]; k.tall_res = knobs[5]; k.tall_dual = knobs[6];
  for (long i = 0; i < n; i++, q += 10, out += 6) {
    ConvParams p = {};
    p.M = q[0]; p.Cout = q[1]; p.Kpad = q[2]; p.Cin = q[3]; p.Cin2 = q[4];
    p.res = q[5] ? &dummy : nullptr; p.in2 = q[6] ? &dummy : nullptr; p.epi = q[7];
    const ConvRoute r = conv_route(p, q[8] != 0, q[9] != 0, k);
    out[0] = r.family; out[1] = r.BM; out[2] = r.BN; out[3] = r.BK; out[4] = r.dual; out[5] = r.line;
  }
}
// the defaults of ConvKnobs, as the library has them when no knob is set
void hx_conv_knob_defaults(int* knobs) {
  const ConvKnobs k;
  knobs[0] = k.dma; knobs[1] = k.line; knobs[2] = k.wide_mintiles; knobs[3] = k.bn64_maxtiles; knobs[4] = k.tall_mintiles; knobs[5] = k.tall_res; knobs[6] = k.tall_dual;
}
}
