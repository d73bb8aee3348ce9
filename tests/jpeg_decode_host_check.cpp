// A stand-alone program over the host half of the JPEG import (tt_jpeg_parse and tt_jpeg_decode_table in
// this_and_that_vdm_amd/csrc/jpeg_host.cpp, with png_host.cpp and lib.cpp), built by tests/test_jpeg_decode_cpu.py with the host
// compiler and -fsanitize=address,undefined and run as a child process.  A baseline file is assembled here from the library's own
// standard tables; it is parsed from a heap buffer of exactly its size, then cut at EVERY length, then with every single byte of its
// headers replaced by 0x00, 0xFF and a random value: each call must return (TT_OK or a refusal with a text) without reading outside
// the buffer.  The decode tables of the four standard tables are checked code by code, and BITS that oversubscribe are refused.
// Exit status 0 and a last line "ok" when every check held.
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

static void segment(std::vector<uint8_t>& f, int marker, const std::vector<uint8_t>& payload) {
  f.push_back(0xff);
  f.push_back((uint8_t)marker);
  f.push_back((uint8_t)((payload.size() + 2) >> 8));
  f.push_back((uint8_t)((payload.size() + 2) & 255));
  f.insert(f.end(), payload.begin(), payload.end());
}

// a 16 x 16 file, 4:2:0 or grey, with the standard tables and a made-up scan; *scan_at: where its entropy-coded bytes begin
static std::vector<uint8_t> make_file(bool grey, size_t* scan_at, size_t* scan_len) {
  std::vector<uint8_t> f = {0xff, 0xd8};
  segment(f, 0xe0, {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
  uint8_t q[128];
  tt_jpeg_quant_tables(75, q);
  for (int t = 0; t < (grey ? 1 : 2); ++t) {
    std::vector<uint8_t> p = {(uint8_t)t};
    for (int i = 0; i < 64; ++i) p.push_back(q[64 * t + i]);                    // (natural order stands in for zig-zag: any bytes do)
    segment(f, 0xdb, p);
  }
  if (grey) segment(f, 0xc0, {8, 0, 16, 0, 16, 1, 1, 0x22, 0});
  else segment(f, 0xc0, {8, 0, 16, 0, 16, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1});
  for (int k = 0; k < (grey ? 2 : 4); ++k) {
    uint8_t bits[16], vals[256];
    uint32_t codes[256];
    int32_t n = 0;
    tt_jpeg_standard_table(k, bits, vals, &n, codes);
    std::vector<uint8_t> p = {(uint8_t)(((k & 1) << 4) | (k >> 1))};
    p.insert(p.end(), bits, bits + 16);
    p.insert(p.end(), vals, vals + n);
    segment(f, 0xc4, p);
  }
  if (grey) segment(f, 0xda, {1, 1, 0x00, 0, 63, 0});
  else segment(f, 0xda, {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
  *scan_at = f.size();
  const uint8_t scan[] = {0x12, 0x34, 0xff, 0x00, 0x56, 0x78, 0x9a, 0xff, 0x00, 0xbc};
  f.insert(f.end(), scan, scan + sizeof(scan));
  *scan_len = sizeof(scan);
  f.push_back(0xff);
  f.push_back(0xd9);
  return f;
}

// parse from a heap buffer of exactly n bytes: the sanitizer sees a read one byte too far
static int parse_exact(const uint8_t* data, size_t n, TtJpegHeader* hd) {
  std::vector<uint8_t> exact(data, data + n);
  return tt_jpeg_parse(exact.data(), (int64_t)n, hd);
}

int main() {
  for (int grey = 0; grey < 2; ++grey) {
    size_t scan_at = 0, scan_len = 0;
    const std::vector<uint8_t> file = make_file(grey != 0, &scan_at, &scan_len);
    TtJpegHeader hd;
    int rc = parse_exact(file.data(), file.size(), &hd);
    CHECK(rc == TT_OK, "the good file: %d %s", rc, tt_last_error());
    CHECK(hd.h == 16 && hd.w == 16 && hd.ch == (grey ? 1 : 3) && hd.subsampling == (grey ? TT_JPEG_444 : TT_JPEG_420), "geometry %d %d %d %d", hd.h, hd.w, hd.ch,
          hd.subsampling);
    CHECK(hd.scan_offset == (int64_t)scan_at && hd.scan_bytes == (int64_t)scan_len, "scan %lld + %lld", (long long)hd.scan_offset, (long long)hd.scan_bytes);
    if (!grey) CHECK(hd.dc_table[0] == 0 && hd.dc_table[1] == 1 && hd.ac_table[2] == 1, "table map");
    // cut at every length: a refusal with a text, never a read behind the buffer
    for (size_t n = 0; n < file.size(); ++n) {
      rc = parse_exact(file.data(), n, &hd);
      CHECK(rc == TT_EINVAL && tt_last_error()[0], "cut at %zu of %zu: rc %d", n, file.size(), rc);
      if (n >= scan_at) CHECK(strstr(tt_last_error(), "ends before EOI"), "cut at %zu: %s", n, tt_last_error());
    }
    // every header byte replaced: any answer, no fault
    for (size_t at = 0; at < scan_at; ++at)
      for (int v = 0; v < 3; ++v) {
        std::vector<uint8_t> m = file;
        m[at] = v == 0 ? 0x00 : (v == 1 ? 0xff : (uint8_t)rnd());
        rc = tt_jpeg_parse(m.data(), (int64_t)m.size(), &hd);
        CHECK(rc == TT_OK || ((rc == TT_EINVAL || rc == TT_EUNSUPPORTED) && tt_last_error()[0]), "byte %zu = %02x: rc %d", at, m[at], rc);
        if (rc == TT_OK) CHECK(hd.scan_offset >= 0 && hd.scan_bytes >= 0 && hd.scan_offset + hd.scan_bytes <= (int64_t)m.size(), "byte %zu: scan outside the file", at);
      }
  }
  TtJpegHeader hd;
  const uint8_t soi[2] = {0xff, 0xd8};
  CHECK(tt_jpeg_parse(nullptr, 4, &hd) == TT_EINVAL && strstr(tt_last_error(), "null data"), "null data");
  CHECK(tt_jpeg_parse(soi, 2, nullptr) == TT_EINVAL && strstr(tt_last_error(), "null header"), "null header");
  CHECK(tt_jpeg_parse(soi, 0, &hd) == TT_EINVAL, "size 0");

  // decode tables: every code of the standard tables found through the words the kernel reads, into exactly 256 words
  for (int k = 0; k < 4; ++k) {
    uint8_t bits[16], vals[256];
    uint32_t codes[256];
    int32_t n = 0;
    tt_jpeg_standard_table(k, bits, vals, &n, codes);
    std::vector<uint32_t> t(TT_JPEG_DECODE_WORDS);
    CHECK(tt_jpeg_decode_table(bits, vals, t.data()) == TT_OK, "decode table %d: %s", k, tt_last_error());
    for (int s = 0; s < 256; ++s) {
      const uint32_t len = codes[s] >> 16, code = codes[s] & 0xffffu;
      if (!len) continue;
      uint32_t sym = 256;
      if (len <= 8) {
        const uint32_t idx = (code << (8 - len)) | (rnd() & ((1u << (8 - len)) - 1u));
        const uint32_t e = (t[idx >> 1] >> (16 * (idx & 1))) & 0xffffu;
        CHECK((e >> 8) == len, "table %d symbol %d: look-ahead length %u, want %u", k, s, e >> 8, len);
        sym = e & 255u;
      } else {
        CHECK((((t[(code >> (len - 8)) >> 1]) >> (16 * ((code >> (len - 8)) & 1))) & 0xffffu) == 0, "table %d symbol %d: a long code in the look-ahead", k, s);
        CHECK((int32_t)code <= (int32_t)t[128 + len], "table %d symbol %d: above MAXCODE", k, s);
        const uint32_t at = (code + t[145 + len]) & 255u;
        sym = (t[192 + (at >> 2)] >> (8 * (at & 3))) & 255u;
      }
      CHECK(sym == (uint32_t)s, "table %d: code of symbol %d decodes to %u", k, s, sym);
    }
  }
  uint8_t bits[16] = {0}, vals[256] = {0};
  std::vector<uint32_t> t(TT_JPEG_DECODE_WORDS);
  bits[0] = 3;                                            // three codes of one bit
  CHECK(tt_jpeg_decode_table(bits, vals, t.data()) == TT_EINVAL && strstr(tt_last_error(), "oversubscribes"), "3 x 1 bit: %s", tt_last_error());
  bits[0] = 2;                                            // complete: accepted
  CHECK(tt_jpeg_decode_table(bits, vals, t.data()) == TT_OK, "2 x 1 bit");
  bits[0] = 1; bits[15] = 255; bits[14] = 255;
  CHECK(tt_jpeg_decode_table(bits, vals, t.data()) == TT_EINVAL && strstr(tt_last_error(), "256 at most"), "511 codes: %s", tt_last_error());
  memset(bits, 0, 16);
  CHECK(tt_jpeg_decode_table(bits, vals, t.data()) == TT_OK, "an empty table");
  for (int i = 0; i < 128; ++i) CHECK(t[i] == 0, "an empty table has a look-ahead entry");
  CHECK(tt_jpeg_decode_table(nullptr, vals, t.data()) == TT_EINVAL && strstr(tt_last_error(), "null bits"), "null bits");
  for (int round = 0; round < 200; ++round) {             // random BITS: refused or usable, never a write outside 256 words
    for (int l = 0; l < 16; ++l) bits[l] = (uint8_t)(rnd() % (l < 4 ? 2 : 6));
    for (int i = 0; i < 256; ++i) vals[i] = (uint8_t)rnd();
    std::vector<uint32_t> exact(TT_JPEG_DECODE_WORDS);
    const int rc = tt_jpeg_decode_table(bits, vals, exact.data());
    CHECK(rc == TT_OK || rc == TT_EINVAL, "random BITS: %d", rc);
  }
  CHECK(tt_jpeg_sequence_bits() == 256 * (int64_t)TT_JPEG_SUBSEQ_BITS, "sequence bits");
  CHECK(tt_jpeg_entropy_ws_bytes(2, 100) == 16 + 16 + 2 * (112 + 16) && tt_jpeg_entropy_ws_bytes(0, 100) == 0 && tt_jpeg_entropy_ws_bytes(1, 1ll << 28) == 0, "ws bytes");

  if (failures) { printf("%d checks failed\n", failures); return 1; }
  printf("ok\n");
  return 0;
}
