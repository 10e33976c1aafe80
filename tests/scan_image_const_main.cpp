// The "does the constant fit the scan image / truncate it" decision of csrc/scan_image.hpp over its edge grid, as a stand-alone host program
// (tests/test_scan_image_const.py builds it with -fsanitize=address,undefined and runs it).  Exit status 0 = every case as expected.
#include <cstdio>
#include "../dataframedbs.jl_amd/csrc/scan_image.hpp"

int main() {
  using namespace dfdb;
  struct Case { int32_t dtype; uint64_t bits; bool fits; uint64_t image; };
  const Case cases[] = {
      {DFDB_I64, (uint64_t)INT64_C(-2147483648), true, 0x80000000ull},  {DFDB_I64, (uint64_t)INT64_C(-2147483649), false, 0},
      {DFDB_I64, (uint64_t)INT64_C(-1), true, 0xffffffffull},          {DFDB_I64, 0, true, 0},
      {DFDB_I64, 899999, true, 899999},                                {DFDB_I64, 2147483647, true, 0x7fffffffull},
      {DFDB_I64, 2147483648ull, false, 0},                             {DFDB_I64, 4294967295ull, false, 0},
      {DFDB_I64, (uint64_t)INT64_MIN, false, 0},                       {DFDB_I64, (uint64_t)INT64_MAX, false, 0},
      {DFDB_I64, 0xffffffff00000000ull, false, 0},                     {DFDB_I64, 0x100000000ull, false, 0},
      {DFDB_U64, 0, true, 0},                                          {DFDB_U64, 40, true, 40},
      {DFDB_U64, 2147483648ull, true, 0x80000000ull},                  {DFDB_U64, 4294967295ull, true, 0xffffffffull},
      {DFDB_U64, 4294967296ull, false, 0},                             {DFDB_U64, UINT64_MAX, false, 0},
      {DFDB_F64, 0, false, 0},                                         {DFDB_I32, 0, false, 0},
  };
  int bad = 0;
  for (const Case& c : cases) {
    uint64_t got = 0xdeadbeefdeadbeefull;
    const bool fits = scan_image_const(c.dtype, c.bits, &got);
    if (fits != c.fits || (fits && got != c.image) || fits != scan_image_fits(c.dtype, c.bits)) {
      std::printf("dtype %d bits %016llx: fits %d image %016llx, expected %d %016llx\n", c.dtype, (unsigned long long)c.bits, (int)fits, (unsigned long long)got, (int)c.fits, (unsigned long long)c.image);
      bad++;
    }
  }
  if (scan_image_dtype(DFDB_I64) != DFDB_I32 || scan_image_dtype(DFDB_U64) != DFDB_U32 || scan_image_dtype(DFDB_F64) != 0 || scan_image_dtype(DFDB_I32) != 0 || scan_image_dtype(DFDB_STRING) != 0) {
    std::printf("scan_image_dtype maps a dtype wrongly\n");
    bad++;
  }
  std::printf("%d cases, %d wrong\n", (int)(sizeof cases / sizeof cases[0]), bad);
  return bad ? 1 : 0;
}
