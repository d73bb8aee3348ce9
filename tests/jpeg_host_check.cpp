// A stand-alone program over the host half of the JPEG export (this_and_that_vdm_amd/csrc/jpeg_host.cpp + png_host.cpp, whose
// package-merge it calls, + lib.cpp), built by tests/test_jpeg_export_cpu.py with the host compiler and -fsanitize=address,undefined and
// run as a child process: tt_jpeg_quant_tables at every quality, the four standard tables, tt_jpeg_optimized_table on random, sparse,
// single-symbol, empty, all-equal and Fibonacci counts into buffers of exactly the stated size (Kraft sum, no all-ones code, lengths,
// cost against the standard table), the size queries, and the refusals.  Exit status 0 and a last line "ok" when every check held.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>

#include "ttvdm.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); ++failures; } } while (0)

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint32_t rnd() {                               // xorshift64*: the same inputs on every run
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}

struct Table {
  std::vector<uint8_t> bits = std::vector<uint8_t>(16), vals = std::vector<uint8_t>(256);      // exactly the stated sizes
  std::vector<uint32_t> codes = std::vector<uint32_t>(256);
  int32_t n = -1;
};

// what every table must be: BITS sums to nvals, a prefix code (Kraft sum <= 1) without the all-ones code, the code table its mirror
static void table_checks(const char* name, const Table& t, int limit) {
  int total = 0;
  uint64_t kraft = 0;
  for (int l = 1; l <= 16; ++l) {
    total += t.bits[l - 1];
    kraft += (uint64_t)t.bits[l - 1] << (16 - l);
    CHECK(l <= limit || t.bits[l - 1] == 0, "%s: %d codes of %d bits, the limit is %d", name, t.bits[l - 1], l, limit);
  }
  CHECK(total == t.n, "%s: BITS sums to %d, nvals %d", name, total, t.n);
  CHECK(kraft < (1ull << 16) || t.n == 0, "%s: Kraft sum %llu / 65536 leaves no room for the reserved code", name, (unsigned long long)kraft);
  uint32_t code = 0;
  int k = 0;
  for (int l = 1; l <= 16; ++l) {
    for (int i = 0; i < t.bits[l - 1]; ++i, ++k, ++code) {
      CHECK(t.codes[t.vals[k]] == (code | (uint32_t)l << 16), "%s: symbol %d has %08x, want code %x of %d bits", name, t.vals[k], t.codes[t.vals[k]], code, l);
      CHECK(code != (1u << l) - 1, "%s: symbol %d has the all-ones code of %d bits", name, t.vals[k], l);
    }
    code <<= 1;
  }
}

static uint64_t cost(const std::vector<uint32_t>& counts, const Table& t) {
  uint64_t c = 0;
  for (int s = 0; s < 256; ++s) c += (uint64_t)counts[s] * (t.codes[s] >> 16);
  return c;
}

static void optimized_case(const char* name, const std::vector<uint32_t>& counts, int standard) {
  Table t;
  const int rc = tt_jpeg_optimized_table(counts.data(), t.bits.data(), t.vals.data(), &t.n, t.codes.data());
  CHECK(rc == TT_OK, "%s: %d %s", name, rc, tt_last_error());
  if (rc != TT_OK) return;
  table_checks(name, t, 15);
  int used = 0;
  for (int s = 0; s < 256; ++s) {
    used += counts[s] != 0;
    CHECK((counts[s] != 0) == ((t.codes[s] >> 16) != 0), "%s: symbol %d count %u length %u", name, s, counts[s], t.codes[s] >> 16);
  }
  CHECK(used == t.n, "%s: %d used symbols, nvals %d", name, used, t.n);
  if (standard >= 0) {
    Table st;
    CHECK(tt_jpeg_standard_table(standard, st.bits.data(), st.vals.data(), &st.n, st.codes.data()) == TT_OK, "%s: standard table", name);
    CHECK(cost(counts, t) <= cost(counts, st), "%s: %llu bits, the standard table takes %llu", name, (unsigned long long)cost(counts, t),
          (unsigned long long)cost(counts, st));
  }
}

int main() {
  // quantiser tables: every quality, into exactly 128 bytes
  for (int q = 1; q <= 100; ++q) {
    std::vector<uint8_t> t(128);
    CHECK(tt_jpeg_quant_tables(q, t.data()) == TT_OK, "quality %d: %s", q, tt_last_error());
    const int s = q < 50 ? 5000 / q : 200 - 2 * q;
    const int first = (16 * s + 50) / 100, want = first < 1 ? 1 : (first > 255 ? 255 : first);
    CHECK(t[0] == want, "quality %d: entry 0 is %d, want %d", q, t[0], want);
    for (int i = 0; i < 128; ++i) CHECK(t[i] >= 1, "quality %d: entry %d is 0", q, i);
  }
  CHECK(tt_jpeg_quant_tables(0, nullptr) == TT_EINVAL, "null tables");
  std::vector<uint8_t> q128(128);
  CHECK(tt_jpeg_quant_tables(0, q128.data()) == TT_EINVAL && strstr(tt_last_error(), "quality = 0"), "quality 0: %s", tt_last_error());
  CHECK(tt_jpeg_quant_tables(101, q128.data()) == TT_EINVAL, "quality 101");

  // the standard tables
  const int sizes[4] = {12, 162, 12, 162};
  for (int k = 0; k < 4; ++k) {
    Table t;
    CHECK(tt_jpeg_standard_table(k, t.bits.data(), t.vals.data(), &t.n, t.codes.data()) == TT_OK, "standard %d: %s", k, tt_last_error());
    CHECK(t.n == sizes[k], "standard %d: %d symbols", k, t.n);
    table_checks("standard", t, 16);
  }
  Table bad;
  CHECK(tt_jpeg_standard_table(4, bad.bits.data(), bad.vals.data(), &bad.n, bad.codes.data()) == TT_EINVAL, "which = 4");
  CHECK(tt_jpeg_standard_table(-1, bad.bits.data(), bad.vals.data(), &bad.n, bad.codes.data()) == TT_EINVAL, "which = -1");
  CHECK(tt_jpeg_standard_table(0, nullptr, bad.vals.data(), &bad.n, bad.codes.data()) == TT_EINVAL && strstr(tt_last_error(), "null bits"), "null bits");

  // optimized tables
  for (int round = 0; round < 8; ++round) {
    std::vector<uint32_t> ac(256, 0), dc(256, 0);
    const int shift = 8 + 3 * round;
    for (int run = 0; run < 16; ++run)
      for (int size = 1; size <= 10; ++size)
        if (rnd() % 4 != 0 || round == 0) ac[run * 16 + size] = (rnd() >> (shift > 31 ? 31 : shift)) >> (run / 2) + (round == 0);
    ac[0x00] = rnd() % 5000 + 1;
    ac[0xF0] = rnd() % 50;
    for (int s = 0; s < 12; ++s) dc[s] = rnd() % (1000 >> (s / 2)) + (s == 0);
    optimized_case("random AC", ac, 1);
    optimized_case("random AC against the chrominance table", ac, 3);
    optimized_case("random DC", dc, 0);
  }
  std::vector<uint32_t> one(256, 0), none(256, 0), all(256, 7), fib(256, 0), eob(256, 0);
  one[0x21] = 9;
  optimized_case("a single symbol", one, -1);
  optimized_case("no symbol", none, -1);
  optimized_case("all 256 equal", all, -1);
  uint32_t a = 1, b = 1;
  for (int s = 0; s < 40; ++s) { fib[s * 5] = a; const uint32_t c = a + b; a = b; b = c; }    // unlimited Huffman depth 39: the limit binds
  optimized_case("fibonacci", fib, -1);
  eob[0] = 1;
  optimized_case("EOB alone, count 1 like the reserved symbol", eob, 1);
  Table t;
  CHECK(tt_jpeg_optimized_table(nullptr, t.bits.data(), t.vals.data(), &t.n, t.codes.data()) == TT_EINVAL && strstr(tt_last_error(), "null counts"), "null counts");
  CHECK(tt_jpeg_optimized_table(one.data(), t.bits.data(), t.vals.data(), nullptr, t.codes.data()) == TT_EINVAL, "null nvals");

  // sizes
  CHECK(tt_jpeg_blocks(8, 24, 3, TT_JPEG_420) == 12 && tt_jpeg_blocks(8, 24, 3, TT_JPEG_444) == 9 && tt_jpeg_blocks(8, 24, 1, TT_JPEG_420) == 3, "blocks of 8 x 24");
  CHECK(tt_jpeg_blocks(576, 1024, 3, TT_JPEG_444) == 27648, "blocks of 576 x 1024");
  CHECK(tt_jpeg_blocks(8, 8, 2, 0) == 0 && tt_jpeg_blocks(8, 8, 4, 0) == 0 && tt_jpeg_blocks(8, 8, 3, 1) == 0 && tt_jpeg_blocks(0, 8, 3, 0) == 0, "refused shapes");
  CHECK(tt_jpeg_scan_bound(1, 1, 1, 0) == 448 && tt_jpeg_scan_bound(1, 1, 5, 0) == 0, "scan bound");
  CHECK(tt_jpeg_scan_ws_bytes(2, 8, 8, 1, 0) == 16 + 16 + 16 + 2 * 224 && tt_jpeg_scan_ws_bytes(0, 8, 8, 1, 0) == 0, "ws bytes");

  if (failures) { printf("%d checks failed\n", failures); return 1; }
  printf("ok\n");
  return 0;
}
