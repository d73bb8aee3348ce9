// A stand-alone program over the host routines of the progressive JPEG import (tt_jpeg_parse_progressive and the size query
// tt_jpeg_entropy_progressive_ws_bytes in this_and_that_vdm_amd/csrc/jpeg_host.cpp, with png_host.cpp and lib.cpp), built by
// tests/test_jpeg_progressive_cpu.py with the host compiler and -fsanitize=address,undefined and run as a child process.  Its arguments
// are good progressive files the test wrote.  Each is parsed from a heap buffer of exactly its size into a scan array of exactly the
// count, then cut at EVERY length, then with every single byte replaced by 0x00, 0xFF and a random value: each call must return (TT_OK
// or a refusal with a text) without reading outside the file or writing outside the array.  Exit status 0 and a last line "ok" when
// every check held.
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

// the two calls a caller makes, on a heap copy of exactly n bytes and a scan array of exactly the count: the sanitizer sees a byte too far
static int parse_exact(const uint8_t* data, size_t n, TtJpegProgressiveHeader* hd, std::vector<TtJpegScan>* scans) {
  std::vector<uint8_t> exact(data, data + n);
  int64_t count = -1;
  int rc = tt_jpeg_parse_progressive(exact.data(), (int64_t)n, hd, nullptr, 0, &count);
  if (rc != TT_OK) return rc;
  CHECK(count >= 1 && count <= TT_JPEG_MAX_SCANS && count == hd->nscans, "a count of %lld", (long long)count);
  scans->assign((size_t)count, TtJpegScan());
  int64_t again = -1;
  rc = tt_jpeg_parse_progressive(exact.data(), (int64_t)n, hd, scans->data(), count, &again);
  CHECK(rc == TT_OK && again == count, "the second call: rc %d, %lld scans after %lld", rc, (long long)again, (long long)count);
  for (int64_t s = 0; s < count; ++s) {
    const TtJpegScan& sc = (*scans)[(size_t)s];
    CHECK(sc.offset >= 0 && sc.bytes >= 0 && sc.offset + sc.bytes <= (int64_t)n, "scan %lld outside the file", (long long)s);
    CHECK(sc.comps >= 1 && sc.comps <= 7 && sc.ss >= 0 && sc.ss <= sc.se && sc.se <= 63 && sc.ah >= 0 && sc.ah <= 14 && sc.al >= 0 && sc.al <= 13,
          "scan %lld: comps %d band %d to %d, Ah %d Al %d", (long long)s, sc.comps, sc.ss, sc.se, sc.ah, sc.al);
  }
  return rc;
}

int main(int argc, char** argv) {
  CHECK(argc > 1, "no files");
  TtJpegProgressiveHeader hd;
  std::vector<TtJpegScan> scans;
  for (int a = 1; a < argc; ++a) {
    std::vector<uint8_t> file;
    FILE* fh = fopen(argv[a], "rb");
    CHECK(fh != nullptr, "cannot open %s", argv[a]);
    if (!fh) continue;
    uint8_t buf[4096];
    for (size_t got; (got = fread(buf, 1, sizeof(buf), fh)) > 0;) file.insert(file.end(), buf, buf + got);
    fclose(fh);
    int rc = parse_exact(file.data(), file.size(), &hd, &scans);
    CHECK(rc == TT_OK, "%s: %d %s", argv[a], rc, tt_last_error());
    if (rc != TT_OK) continue;
    const int64_t count = (int64_t)scans.size();
    // a cap below the count and null pointers are refused by name; nothing is written behind the cap
    if (count > 1) {
      std::vector<TtJpegScan> fewer((size_t)count - 1);
      int64_t got = 0;
      CHECK(tt_jpeg_parse_progressive(file.data(), (int64_t)file.size(), &hd, fewer.data(), count - 1, &got) == TT_EINVAL && strstr(tt_last_error(), "scan_cap too small"),
            "cap %lld: %s", (long long)(count - 1), tt_last_error());
    }
    int64_t got = 0;
    CHECK(tt_jpeg_parse_progressive(nullptr, 4, &hd, nullptr, 0, &got) == TT_EINVAL && strstr(tt_last_error(), "null data"), "null data");
    CHECK(tt_jpeg_parse_progressive(file.data(), (int64_t)file.size(), nullptr, nullptr, 0, &got) == TT_EINVAL && strstr(tt_last_error(), "null header"), "null header");
    CHECK(tt_jpeg_parse_progressive(file.data(), (int64_t)file.size(), &hd, nullptr, 0, nullptr) == TT_EINVAL && strstr(tt_last_error(), "null nscans"), "null nscans");
    CHECK(tt_jpeg_parse_progressive(file.data(), 0, &hd, nullptr, 0, &got) == TT_EINVAL && strstr(tt_last_error(), "size = 0"), "size 0");
    // the baseline parsers keep refusing it
    TtJpegHeader base;
    CHECK(tt_jpeg_parse(file.data(), (int64_t)file.size(), &base) == TT_EUNSUPPORTED && strstr(tt_last_error(), "progressive"), "tt_jpeg_parse: %s", tt_last_error());
    // cut at every length: a refusal with a text, never a read behind the buffer
    for (size_t n = 0; n < file.size(); ++n) {
      rc = parse_exact(file.data(), n, &hd, &scans);
      CHECK((rc == TT_EINVAL || rc == TT_EUNSUPPORTED) && tt_last_error()[0], "%s cut at %zu of %zu: rc %d", argv[a], n, file.size(), rc);
    }
    // every byte replaced: any answer, no fault, scans inside the file (parse_exact checks them)
    for (size_t at = 0; at < file.size(); ++at)
      for (int v = 0; v < 3; ++v) {
        std::vector<uint8_t> m = file;
        m[at] = v == 0 ? 0x00 : (v == 1 ? 0xff : (uint8_t)rnd());
        rc = parse_exact(m.data(), m.size(), &hd, &scans);
        CHECK(rc == TT_OK || ((rc == TT_EINVAL || rc == TT_EUNSUPPORTED) && tt_last_error()[0]), "%s byte %zu = %02x: rc %d", argv[a], at, m[at], rc);
      }
    // the size query: grows with the scans, 0 for what the entry point refuses
    const int64_t ws = tt_jpeg_entropy_progressive_ws_bytes(2, (int32_t)count, 1000, hd.h, hd.w, hd.ch, hd.subsampling);
    CHECK(ws >= tt_jpeg_entropy_ws_bytes((int32_t)(2 * count), 1000) + 12 * 2 * tt_jpeg_blocks(hd.h, hd.w, hd.ch, hd.subsampling) && ws % 16 == 0, "ws %lld", (long long)ws);
    CHECK(tt_jpeg_entropy_progressive_ws_bytes(0, 1, 1000, hd.h, hd.w, hd.ch, hd.subsampling) == 0 &&
              tt_jpeg_entropy_progressive_ws_bytes(1, 0, 1000, hd.h, hd.w, hd.ch, hd.subsampling) == 0 &&
              tt_jpeg_entropy_progressive_ws_bytes(1, TT_JPEG_MAX_SCANS + 1, 1000, hd.h, hd.w, hd.ch, hd.subsampling) == 0 &&
              tt_jpeg_entropy_progressive_ws_bytes(300, 256, 1000, hd.h, hd.w, hd.ch, hd.subsampling) == 0 &&
              tt_jpeg_entropy_progressive_ws_bytes(1, 1, 1ll << 28, hd.h, hd.w, hd.ch, hd.subsampling) == 0 &&
              tt_jpeg_entropy_progressive_ws_bytes(1, 1, 1000, 0, hd.w, hd.ch, hd.subsampling) == 0,
          "refused arguments");
  }
  if (failures) { printf("%d checks failed\n", failures); return 1; }
  printf("ok\n");
  return 0;
}
