// A stand-alone program over the host routines of the JPEG restart intervals (tt_jpeg_parse_spans and the size queries
// tt_jpeg_scan_bound_restart / tt_jpeg_scan_restart_ws_bytes in this_and_that_vdm_amd/csrc/jpeg_host.cpp, with png_host.cpp and lib.cpp),
// built by tests/test_jpeg_restart_cpu.py with the host compiler and -fsanitize=address,undefined and run as a child process.  A 48 x 16
// 4:2:0 file (3 MCUs) with DRI 1 and a made-up scan of three spans is assembled here; it is parsed from a heap buffer of exactly its
// size into span arrays of exactly the count, then cut at EVERY length, then with every single byte of its headers and of its scan
// replaced by 0x00, 0xFF and a random value: each call must return (TT_OK or a refusal with a text) without reading outside the file
// or writing outside the arrays.  Exit status 0 and a last line "ok" when every check held.
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

static void segment(std::vector<uint8_t>& f, int marker, const std::vector<uint8_t>& payload) {
  f.push_back(0xff);
  f.push_back((uint8_t)marker);
  f.push_back((uint8_t)((payload.size() + 2) >> 8));
  f.push_back((uint8_t)((payload.size() + 2) & 255));
  f.insert(f.end(), payload.begin(), payload.end());
}

struct Span { int64_t at, len; };

// 48 x 16, 4:2:0, the standard tables, DRI `ri` before SOS (ri < 0: no DRI segment), a made-up scan whose spans are returned
static std::vector<uint8_t> make_file(int ri, bool markers, size_t* scan_at, std::vector<Span>* spans) {
  std::vector<uint8_t> f = {0xff, 0xd8};
  segment(f, 0xe0, {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
  uint8_t q[128];
  tt_jpeg_quant_tables(75, q);
  for (int t = 0; t < 2; ++t) {
    std::vector<uint8_t> p = {(uint8_t)t};
    for (int i = 0; i < 64; ++i) p.push_back(q[64 * t + i]);
    segment(f, 0xdb, p);
  }
  segment(f, 0xc0, {8, 0, 16, 0, 48, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1});
  for (int k = 0; k < 4; ++k) {
    uint8_t bits[16], vals[256];
    uint32_t codes[256];
    int32_t n = 0;
    tt_jpeg_standard_table(k, bits, vals, &n, codes);
    std::vector<uint8_t> p = {(uint8_t)(((k & 1) << 4) | (k >> 1))};
    p.insert(p.end(), bits, bits + 16);
    p.insert(p.end(), vals, vals + n);
    segment(f, 0xc4, p);
  }
  if (ri >= 0) segment(f, 0xdd, {(uint8_t)(ri >> 8), (uint8_t)(ri & 255)});
  segment(f, 0xda, {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
  *scan_at = f.size();
  spans->clear();
  const std::vector<std::vector<uint8_t>> parts = {{0x12, 0x34, 0xff, 0x00}, {0x56, 0xff, 0x00}, {0x9a, 0xbc, 0xde}};
  for (size_t k = 0; k < parts.size(); ++k) {
    if (markers || k == 0) spans->push_back({(int64_t)f.size(), 0});
    f.insert(f.end(), parts[k].begin(), parts[k].end());
    spans->back().len = (int64_t)f.size() - spans->back().at;
    if (markers && k + 1 < parts.size()) { f.push_back(0xff); f.push_back((uint8_t)(0xd0 + k)); }
  }
  f.push_back(0xff);
  f.push_back(0xd9);
  return f;
}

// the two calls a caller makes, on a heap copy of exactly n bytes and span arrays of exactly the count: the sanitizer sees a byte too far
static int parse_exact(const uint8_t* data, size_t n, TtJpegHeader* hd, int32_t* ri, std::vector<int64_t>* offs, std::vector<int64_t>* lens) {
  std::vector<uint8_t> exact(data, data + n);
  int64_t count = -1;
  int rc = tt_jpeg_parse_spans(exact.data(), (int64_t)n, hd, ri, nullptr, nullptr, 0, &count);
  if (rc != TT_OK) return rc;
  CHECK(count >= 1, "a count of %lld", (long long)count);
  offs->assign((size_t)count, -1);
  lens->assign((size_t)count, -1);
  int64_t again = -1;
  rc = tt_jpeg_parse_spans(exact.data(), (int64_t)n, hd, ri, offs->data(), lens->data(), count, &again);
  CHECK(rc == TT_OK && again == count, "the second call: rc %d, %lld spans after %lld", rc, (long long)again, (long long)count);
  for (int64_t s = 0; s < count; ++s)
    CHECK((*offs)[s] >= hd->scan_offset && (*lens)[s] >= 0 && (*offs)[s] + (*lens)[s] <= hd->scan_offset + hd->scan_bytes, "span %lld outside the scan", (long long)s);
  return rc;
}

int main() {
  size_t scan_at = 0;
  std::vector<Span> want;
  TtJpegHeader hd;
  int32_t ri = -1;
  std::vector<int64_t> offs, lens;
  const std::vector<uint8_t> file = make_file(1, true, &scan_at, &want);
  int rc = parse_exact(file.data(), file.size(), &hd, &ri, &offs, &lens);
  CHECK(rc == TT_OK, "the good file: %d %s", rc, tt_last_error());
  CHECK(hd.h == 16 && hd.w == 48 && hd.ch == 3 && hd.subsampling == TT_JPEG_420 && ri == 1, "geometry %d %d %d %d, interval %d", hd.h, hd.w, hd.ch, hd.subsampling, ri);
  CHECK(hd.scan_offset == (int64_t)scan_at && hd.scan_offset + hd.scan_bytes + 2 == (int64_t)file.size(), "scan %lld + %lld", (long long)hd.scan_offset, (long long)hd.scan_bytes);
  CHECK(offs.size() == want.size(), "%zu spans", offs.size());
  for (size_t s = 0; s < want.size() && s < offs.size(); ++s) CHECK(offs[s] == want[s].at && lens[s] == want[s].len, "span %zu: %lld + %lld", s, (long long)offs[s], (long long)lens[s]);
  // a cap below the count is refused by name; the arrays go together
  int64_t count = 0;
  std::vector<int64_t> two(2), two2(2);
  CHECK(tt_jpeg_parse_spans(file.data(), (int64_t)file.size(), &hd, &ri, two.data(), two2.data(), 2, &count) == TT_EINVAL && strstr(tt_last_error(), "span_cap too small"),
        "cap 2: %s", tt_last_error());
  CHECK(tt_jpeg_parse_spans(file.data(), (int64_t)file.size(), &hd, &ri, two.data(), nullptr, 2, &count) == TT_EINVAL && strstr(tt_last_error(), "go together"), "one array");
  CHECK(tt_jpeg_parse_spans(file.data(), (int64_t)file.size(), &hd, nullptr, nullptr, nullptr, 0, &count) == TT_EINVAL && strstr(tt_last_error(), "null restart_interval"), "null ri");
  CHECK(tt_jpeg_parse_spans(file.data(), (int64_t)file.size(), &hd, &ri, nullptr, nullptr, 0, nullptr) == TT_EINVAL && strstr(tt_last_error(), "null nspans"), "null nspans");
  CHECK(tt_jpeg_parse_spans(nullptr, 4, &hd, &ri, nullptr, nullptr, 0, &count) == TT_EINVAL && strstr(tt_last_error(), "null data"), "null data");
  CHECK(tt_jpeg_parse_spans(file.data(), (int64_t)file.size(), nullptr, &ri, nullptr, nullptr, 0, &count) == TT_EINVAL && strstr(tt_last_error(), "null header"), "null header");
  // a file without markers: one span, tt_jpeg_parse's scan range
  {
    size_t at0 = 0;
    std::vector<Span> one;
    for (int dri = -1; dri <= 0; ++dri) {
      const std::vector<uint8_t> plain = make_file(dri, false, &at0, &one);
      TtJpegHeader h1, h2;
      rc = parse_exact(plain.data(), plain.size(), &h1, &ri, &offs, &lens);
      CHECK(rc == TT_OK && ri == 0 && offs.size() == 1, "no markers (DRI %d): rc %d %s", dri, rc, tt_last_error());
      CHECK(tt_jpeg_parse(plain.data(), (int64_t)plain.size(), &h2) == TT_OK, "tt_jpeg_parse: %s", tt_last_error());
      if (offs.size() == 1) CHECK(offs[0] == h2.scan_offset && lens[0] == h2.scan_bytes, "the one span is not the scan range");
    }
    // markers in such a file, a wrong count, a wrong number: by name
    const std::vector<uint8_t> stray = make_file(-1, true, &at0, &one), zero = make_file(0, true, &at0, &one), few = make_file(2, true, &at0, &one);
    CHECK(parse_exact(stray.data(), stray.size(), &hd, &ri, &offs, &lens) == TT_EINVAL && strstr(tt_last_error(), "with no DRI segment"), "stray: %s", tt_last_error());
    CHECK(parse_exact(zero.data(), zero.size(), &hd, &ri, &offs, &lens) == TT_EINVAL && strstr(tt_last_error(), "DRI segment says 0"), "zero: %s", tt_last_error());
    CHECK(parse_exact(few.data(), few.size(), &hd, &ri, &offs, &lens) == TT_EINVAL && strstr(tt_last_error(), "2 restart markers where"), "count: %s", tt_last_error());
    std::vector<uint8_t> order = file;
    order[(size_t)want[1].at - 1] = 0xd3;
    CHECK(parse_exact(order.data(), order.size(), &hd, &ri, &offs, &lens) == TT_EINVAL && strstr(tt_last_error(), "is RST3 where RST0 is due"), "order: %s", tt_last_error());
    CHECK(tt_jpeg_parse(file.data(), (int64_t)file.size(), &hd) == TT_EUNSUPPORTED && strstr(tt_last_error(), "restart"), "tt_jpeg_parse keeps refusing: %s", tt_last_error());
  }
  // cut at every length: a refusal with a text, never a read behind the buffer
  for (size_t n = 0; n < file.size(); ++n) {
    rc = parse_exact(file.data(), n, &hd, &ri, &offs, &lens);
    CHECK(rc == TT_EINVAL && tt_last_error()[0], "cut at %zu of %zu: rc %d", n, file.size(), rc);
    if (n >= scan_at) CHECK(strstr(tt_last_error(), "ends before EOI"), "cut at %zu: %s", n, tt_last_error());
  }
  // every byte of the headers and of the scan replaced: any answer, no fault, spans inside the scan (parse_exact checks them)
  for (size_t at = 0; at < file.size(); ++at)
    for (int v = 0; v < 3; ++v) {
      std::vector<uint8_t> m = file;
      m[at] = v == 0 ? 0x00 : (v == 1 ? 0xff : (uint8_t)rnd());
      rc = parse_exact(m.data(), m.size(), &hd, &ri, &offs, &lens);
      CHECK(rc == TT_OK || ((rc == TT_EINVAL || rc == TT_EUNSUPPORTED) && tt_last_error()[0]), "byte %zu = %02x: rc %d", at, m[at], rc);
      if (rc == TT_OK) CHECK(hd.scan_offset >= 0 && hd.scan_bytes >= 0 && hd.scan_offset + hd.scan_bytes <= (int64_t)m.size(), "byte %zu: scan outside the file", at);
    }

  // the size queries: interval 0 is tt_jpeg_scan's; a marker takes 4 stuffed bytes or more; refused arguments give 0
  for (int sub = 0; sub <= 2; sub += 2) {
    const int64_t plain = tt_jpeg_scan_bound(37, 53, 3, sub), blocks = tt_jpeg_blocks(37, 53, 3, sub), mcus = blocks / (sub ? 6 : 3);
    CHECK(tt_jpeg_scan_bound_restart(37, 53, 3, sub, 0) == plain, "bound at interval 0");
    CHECK(tt_jpeg_scan_restart_ws_bytes(3, 37, 53, 3, sub, 0) == tt_jpeg_scan_ws_bytes(3, 37, 53, 3, sub), "ws at interval 0");
    for (int r = 1; r <= (int)mcus + 1; ++r) {
      const int64_t markers = (mcus + r - 1) / r - 1, b = tt_jpeg_scan_bound_restart(37, 53, 3, sub, r);
      CHECK(b % 16 == 0 && b >= plain + 4 * markers && b / 2 >= plain / 2 + 3 * markers, "bound at interval %d: %lld", r, (long long)b);
      CHECK(tt_jpeg_scan_restart_ws_bytes(3, 37, 53, 3, sub, r) >= tt_jpeg_scan_ws_bytes(3, 37, 53, 3, sub) + 3 * 3 * markers, "ws at interval %d", r);
    }
    CHECK(tt_jpeg_scan_bound_restart(37, 53, 3, sub, 65536) == 0 && tt_jpeg_scan_bound_restart(37, 53, 3, sub, -1) == 0 && tt_jpeg_scan_bound_restart(0, 53, 3, sub, 1) == 0,
          "refused arguments");
    CHECK(tt_jpeg_scan_restart_ws_bytes(3, 37, 53, 3, sub, 65536) == 0 && tt_jpeg_scan_restart_ws_bytes(0, 37, 53, 3, sub, 1) == 0, "refused arguments (ws)");
  }

  if (failures) { printf("%d checks failed\n", failures); return 1; }
  printf("ok\n");
  return 0;
}
