// Known answers of the dropout mask for tests/dropout_model.py: a HOST build of common.h's own functions
// (xf_make_dropout, xf_drop_resolve, xf_drop_rowkey, xf_keep_scale_rc, kDropColMul). No device code is launched and no HIP
// API is called, so it runs on a machine without a GPU. It prints the JSON kept as tests/golden/dropout_model.json:
//
//   hipcc --offload-arch=gfx950 -O1 -std=c++17 -I include -I transformer-recommenders_amd/csrc \
//         scripts/probe/dropout_host_model.hip -o /tmp/dropout_host_model && /tmp/dropout_host_model \
//         > tests/golden/dropout_model.json
//
// Per (p, seed, site) case: key, threshold, the fp32 scale's bit pattern, and over the 300 x 130 elements
// (row = 977 r, col = c): the kept count, an order-sensitive FNV-1a signature of the keep bits, and the first row as a string.
#include "common.h"

#include <cstdio>
#include <cstring>

static void emit_case(float p, uint64_t seed, uint32_t site, bool last) {
  XfDropout d = xf_make_dropout(p, XfSeed(seed), site);
  uint32_t scale_bits;
  memcpy(&scale_bits, &d.scale, 4);
  uint32_t kept = 0, sig = 2166136261u;
  char row0[131];
  for (uint32_t r = 0; r < 300; ++r) {
    const uint32_t rk = xf_drop_rowkey(d, r * 977u);
    for (uint32_t c = 0; c < 130; ++c) {
      const uint32_t k = !d.on || xf_keep_scale_rc(d, rk, c * kDropColMul) != 0.f;
      kept += k;
      sig = (sig ^ k) * 16777619u;
      if (r == 0) row0[c] = k ? '1' : '0';
    }
  }
  row0[130] = 0;
  float p32 = p;
  uint32_t p_bits;
  memcpy(&p_bits, &p32, 4);
  printf("  {\"p_bits\": %u, \"seed\": %llu, \"site\": %u, \"key\": %u, \"thresh\": %u, \"scale_bits\": %u, \"kept\": %u, "
         "\"sig\": %u, \"row0\": \"%s\"}%s\n",
         p_bits, (unsigned long long)seed, site, d.key, d.thresh, scale_bits, kept, sig, row0, last ? "" : ",");
}

int main() {
  const float ps[3] = {0.1f, 0.25f, 0.3f};
  const uint64_t seeds[2] = {5ull, 6018027440424182934ull};
  const uint32_t sites[3] = {0, 3, 9};
  printf("{\"rows\": 300, \"row_mul\": 977, \"cols\": 130,\n \"cases\": [\n");
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 2; ++j)
      for (int k = 0; k < 3; ++k) emit_case(ps[i], seeds[j], sites[k], i == 2 && j == 1 && k == 2);
  printf(" ],\n \"steps\": [\n");
  const uint32_t steps[4] = {0, 1, 41, 4000000000u};
  for (int j = 0; j < 2; ++j)
    for (int s = 0; s < 4; ++s) {
      XfDropout d = xf_make_dropout(0.1f, XfSeed(seeds[j], &steps[s]), 3);
      d = xf_drop_resolve(d);
      printf("  {\"seed\": %llu, \"site\": 3, \"step\": %u, \"key\": %u}%s\n", (unsigned long long)seeds[j], steps[s], d.key,
             (j == 1 && s == 3) ? "" : ",");
    }
  printf(" ]}\n");
  return 0;
}
