// A stand-alone program over the host half of the PNG export (this_and_that_vdm_amd/csrc/png_host.cpp + lib.cpp), built by
// tests/test_png_export_cpu.py with the host compiler and -fsanitize=address,undefined and run as a child process: tt_png_code_lengths
// on random, single-symbol, all-equal and Fibonacci counts at both limits (lengths within the limit, Kraft sum exactly 1, no cost above
// a flat code's), tt_png_block_header on those and on sparse lengths with long zero runs, into buffers of exactly the stated size, and
// tt_png_plan over a batch of records, with the refusals of all three.  Exit status 0 and a last line "ok" when every check held.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>

#include "ttvdm.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); ++failures; } } while (0)

static uint64_t rng_state = 0x13198A2E03707344ull;
static uint32_t rnd() {                               // xorshift64*: the same inputs on every run
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}

static void lengths_case(const char* name, const std::vector<uint32_t>& counts, int limit) {
  const int nsym = (int)counts.size();
  std::vector<uint8_t> len((size_t)nsym);                // exactly nsym bytes: an overrun is the sanitizer's to find
  const int rc = tt_png_code_lengths(counts.data(), nsym, limit, len.data());
  CHECK(rc == TT_OK, "%s (limit %d): %d %s", name, limit, rc, tt_last_error());
  if (rc != TT_OK) return;
  uint64_t kraft = 0, cost = 0, total = 0;
  int used = 0, flat = 0;
  for (int s = 0; s < nsym; ++s) {
    CHECK((counts[s] != 0) == (len[s] != 0), "%s: symbol %d count %u length %d", name, s, counts[s], len[s]);
    CHECK(len[s] <= limit, "%s: length %d above the limit %d", name, len[s], limit);
    if (len[s]) { kraft += 1ull << (limit - len[s]); ++used; }
    cost += (uint64_t)counts[s] * len[s];
    total += counts[s];
  }
  while ((1 << flat) < used) ++flat;
  if (used >= 2) CHECK(kraft == 1ull << limit, "%s (limit %d): Kraft sum %llu / %llu", name, limit, (unsigned long long)kraft, 1ull << limit);
  CHECK(cost <= total * (uint64_t)(flat ? flat : 1), "%s: cost %llu above a flat code's", name, (unsigned long long)cost);
}

static void header_case(const char* name, std::vector<uint32_t> counts) {
  counts.resize(TT_PNG_SYMS, 0);
  counts[256] = 1;
  std::vector<uint8_t> len(TT_PNG_SYMS);
  int rc = tt_png_code_lengths(counts.data(), TT_PNG_SYMS, 15, len.data());
  CHECK(rc == TT_OK, "%s: %d %s", name, rc, tt_last_error());
  std::vector<uint32_t> header(TT_PNG_HEADER_WORDS);
  int64_t bits = -1;
  rc = tt_png_block_header(counts.data(), len.data(), header.data(), TT_PNG_HEADER_WORDS, &bits);
  CHECK(rc == TT_OK, "%s: header: %d %s", name, rc, tt_last_error());
  CHECK(header[0] >= 17 + 12 && header[0] <= 2083, "%s: %u header bits", name, header[0]);
  CHECK(bits > (int64_t)header[0], "%s: %lld stripe bits", name, (long long)bits);
  for (uint32_t b = header[0]; b < (TT_PNG_HEADER_WORDS - 1) * 32u; ++b)
    CHECK(!((header[1 + b / 32] >> (b % 32)) & 1u), "%s: bit %u behind the header is set", name, b);
  rc = tt_png_block_header(counts.data(), len.data(), header.data(), TT_PNG_HEADER_WORDS - 1, &bits);
  CHECK(rc == TT_EINVAL && strstr(tt_last_error(), "cap too small"), "%s: a short buffer: %d %s", name, rc, tt_last_error());
}

int main() {
  for (int limit : {15, 7}) {
    const int nsym = limit == 15 ? TT_PNG_SYMS : 19;
    for (int round = 0; round < 20; ++round) {
      std::vector<uint32_t> c((size_t)nsym);
      for (auto& v : c) v = rnd() % 4 ? rnd() % (1u << (rnd() % 16)) : 0;
      c[rnd() % nsym] = 1 + rnd() % 100;
      lengths_case("random", c, limit);
    }
    std::vector<uint32_t> one((size_t)nsym, 0);
    one[nsym / 2] = 9;
    lengths_case("one symbol", one, limit);
    lengths_case("all equal", std::vector<uint32_t>((size_t)nsym, 7), limit);
    std::vector<uint32_t> fib((size_t)nsym, 0);
    for (int i = 0; i < (limit == 15 ? 21 : 12); ++i) fib[i] = i < 2 ? 1 : fib[i - 1] + fib[i - 2];
    lengths_case("fibonacci", fib, limit);
  }
  {
    std::vector<uint32_t> c(TT_PNG_SYMS, 3);
    uint8_t len[TT_PNG_SYMS];
    CHECK(tt_png_code_lengths(nullptr, 5, 15, len) == TT_EINVAL, "null counts");
    CHECK(tt_png_code_lengths(c.data(), 0, 15, len) == TT_EINVAL, "nsym 0");
    CHECK(tt_png_code_lengths(c.data(), 287, 15, len) == TT_EINVAL, "nsym 287");
    CHECK(tt_png_code_lengths(c.data(), 19, 16, len) == TT_EINVAL, "limit 16");
    CHECK(tt_png_code_lengths(c.data(), TT_PNG_SYMS, 8, len) == TT_EINVAL, "286 symbols in 8 bits");
    std::vector<uint32_t> z(19, 0);
    CHECK(tt_png_code_lengths(z.data(), 19, 7, len) == TT_EINVAL, "no used symbol");
  }
  header_case("one literal", {5});
  header_case("HLIT 257, zeros of 138 and 11", [] { std::vector<uint32_t> c(256, 0); c[0] = 4; c[149] = 9; return c; }());
  header_case("all 286 equal", std::vector<uint32_t>(TT_PNG_SYMS, 11));
  header_case("random", [] { std::vector<uint32_t> c(TT_PNG_SYMS); for (auto& v : c) v = rnd() % 3 ? rnd() % 2000 : 0; return c; }());
  header_case("fibonacci", [] { std::vector<uint32_t> c(40, 0); for (int i = 0; i < 21; ++i) c[i] = i < 2 ? 1 : c[i - 1] + c[i - 2]; return c; }());
  {
    const int64_t n = 5;
    std::vector<uint32_t> rec((size_t)n * TT_PNG_RECORD_WORDS, 0), tab((size_t)n * TT_PNG_TABLE_WORDS), hdr((size_t)n * TT_PNG_HEADER_WORDS);
    for (int64_t i = 0; i < n; ++i) {
      uint32_t* r = rec.data() + i * TT_PNG_RECORD_WORDS;
      for (int k = 0; k < 300; ++k) ++r[rnd() % (i == 0 ? 2 : TT_PNG_SYMS)];
      r[256] = 1;
    }
    int64_t total = -1;
    int rc = tt_png_plan(rec.data(), n, tab.data(), hdr.data(), &total);
    CHECK(rc == TT_OK && total > 0, "plan: %d %s", rc, tt_last_error());
    int64_t prev = -1;
    for (int64_t i = 0; i < n; ++i) {
      const uint32_t* t = tab.data() + i * TT_PNG_TABLE_WORDS;
      const int64_t off = (int64_t)(((uint64_t)t[287] << 32) | t[286]);
      CHECK(off > prev && off < total, "plan: offset %lld of stripe %lld", (long long)off, (long long)i);
      prev = off;
      for (int s = 0; s < TT_PNG_SYMS; ++s) CHECK((t[s] >> 16) <= 15 && (t[s] & 0xffffu) < (1u << (t[s] >> 16)), "plan: entry %d of stripe %lld", s, (long long)i);
    }
    rec[256] = 2;
    CHECK(tt_png_plan(rec.data(), n, tab.data(), hdr.data(), &total) == TT_EINVAL, "plan: a record without its end of block");
    CHECK(tt_png_plan(rec.data(), 0, tab.data(), hdr.data(), &total) == TT_EINVAL, "plan: no stripe");
    CHECK(tt_png_plan(nullptr, n, tab.data(), hdr.data(), &total) == TT_EINVAL, "plan: null records");
  }
  CHECK(tt_png_stream_bytes(9, 97, 3) == 9 * (1 + 97 * 3) && tt_png_frame_stride(9, 97, 3) % 16 == 0 && tt_png_stripes(576, 1024, 3) == 55, "sizes");
  CHECK(tt_png_stream_bytes(0, 5, 3) == 0 && tt_png_stream_bytes(5, 5, 5) == 0, "sizes of a refused shape");
  if (failures) { printf("%d checks failed\n", failures); return 1; }
  printf("ok\n");
  return 0;
}
