// cmp_plan_check.cpp -- TEST INFRASTRUCTURE: a stand-alone program around the pure-host derivation of element_cmp's integer
// (pbc_amd/csrc/cmp_plan.h), built with -fsanitize=address,undefined by tests/test_cmp_cpu.py.  For every parameter file
// named on the command line it prints "<file> <quotient_cmp in hex> <walked integer in hex>" ("-" where the type has
// none).  Not part of the product.
#include <stdio.h>

#include <string>
#include <vector>

#include "../../pbc_amd/csrc/cmp_plan.h"

static std::string hex(const std::vector<uint8_t> &v) {
  static const char *d = "0123456789abcdef";
  std::string s;
  for (uint8_t b : v) { s += d[b >> 4]; s += d[b & 15]; }
  return s.empty() ? "-" : s;
}

int main(int argc, char **argv) {
  for (int i = 1; i < argc; i++) {
    FILE *f = fopen(argv[i], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[i]); return 2; }
    std::string text;
    char buf[4096];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, got);
    fclose(f);
    std::vector<uint8_t> c0, c1;
    const bool ok0 = pbc_host::cmp_quotient(text.data(), text.size(), 0, c0), ok1 = pbc_host::cmp_quotient(text.data(), text.size(), 1, c1);
    if (ok0 != ok1) { fprintf(stderr, "%s: the two derivations disagree\n", argv[i]); return 1; }
    printf("%s %s %s\n", argv[i], hex(c0).c_str(), hex(c1).c_str());
  }
  return 0;
}
