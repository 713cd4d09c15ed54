// v3p_main.cpp -- TEST-ONLY stand-alone host program: every helper of the pair-of-3-vectors type (csrc/env_core.hpp `v3p`) against the scalar
// v3 helper it replaces, bit for bit, on the host lane emulation (tests/host_emulation/lanes_cpu.hpp: a vf is four lanes, so every round is
// four cases).  usage: v3p_main [rounds]   -> prints the number of cases, exit status 1 at the first mismatch.
#include "lanes_cpu.hpp"

#include "env_core.hpp"

#include <cstdio>
#include <cstdlib>

using namespace irrl;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t next_u32() {
  g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
  return (uint32_t)(g_state >> 32);
}
// one float: 1 in 8 a signed zero, 1 in 8 at the ends of the range (+-2^-30, +-2^30: every product and sum of the helpers stays normal and
// finite), otherwise a random mantissa with an exponent uniform in -30 .. 30
static float next_float() {
  const uint32_t r = next_u32(), sign = r & 0x80000000u, kind = (r >> 8) & 7u;
  uint32_t bits;
  if (kind == 0) bits = sign;
  else if (kind == 1) bits = sign | ((uint32_t)(((r >> 4) & 1u) ? 127 + 30 : 127 - 30) << 23);
  else bits = sign | ((uint32_t)(127 - 30 + (int)(next_u32() % 61u)) << 23) | (next_u32() & 0x7FFFFFu);
  float f;
  std::memcpy(&f, &bits, 4);
  return f;
}
static vf rvf() { vf r; for (int i = 0; i < W; i++) r.v[i] = next_float(); return r; }
static v3 rv3() { v3 r; r.x = rvf(); r.y = rvf(); r.z = rvf(); return r; }

static long g_cases = 0;
static bool same(vf a, vf b) { return std::memcmp(a.v, b.v, sizeof(a.v)) == 0; }
static bool same3(v3 a, v3 b) { return same(a.x, b.x) && same(a.y, b.y) && same(a.z, b.z); }
static void check(const char *what, v3p got, v3 want_lo, v3 want_hi) {
  g_cases += W;
  if (same3(lo3(got), want_lo) && same3(hi3(got), want_hi)) return;
  std::printf("MISMATCH in %s\n", what);
  std::exit(1);
}

int main(int argc, char **argv) {
  const int rounds = argc > 1 ? std::atoi(argv[1]) : 1000;
  for (int it = 0; it < rounds; it++) {
    const v3 a = rv3(), b = rv3(), c = rv3(), d = rv3();
    const vf s = rvf();
    sym3 A;
    A.xx = rvf(); A.xy = rvf(); A.xz = rvf(); A.yy = rvf(); A.yz = rvf(); A.zz = rvf();
    rot3 R;
    R.r0 = rv3(); R.r1 = rv3(); R.r2 = rv3();
    const v3p ab = pk3(a, b), cd = pk3(c, d);
    check("pk3 / lo3 / hi3", ab, a, b);
    check("v3p + v3p", ab + cd, a + c, b + d);
    check("v3p - v3p", ab - cd, a - c, b - d);
    check("s * v3p", s * ab, s * a, s * b);
    check("cross(v3, v3p)", cross(c, ab), cross(c, a), cross(c, b));
    check("cross(v3p, v3)", cross(ab, c), cross(a, c), cross(b, c));
    check("cross(v3p, v3p)", cross(ab, cd), cross(a, c), cross(b, d));
    check("mul(sym3, v3p)", mul(A, ab), mul(A, a), mul(A, b));
    check("rot_mul(R, v3p)", rot_mul(R, ab), rot_mul(R, a), rot_mul(R, b));
    check("rot_tmul(R, v3p)", rot_tmul(R, ab), rot_tmul(R, a), rot_tmul(R, b));
    const vf u[6] = {a.x, a.y, a.z, b.x, b.y, b.z};
    vf w[6];
    check("pk6", pk6(u), a, b);
    unpk6(cd, w);
    check("unpk6", pk3(mk3(w[0], w[1], w[2]), mk3(w[3], w[4], w[5])), c, d);
  }
  std::printf("v3p: %ld cases, all helpers bit for bit\n", g_cases);
  return 0;
}
