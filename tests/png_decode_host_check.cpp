// A stand-alone program over the host routine of the PNG import (tt_png_parse in this_and_that_vdm_amd/csrc/png_host.cpp, with lib.cpp),
// built by tests/test_png_decode_cpu.py with the host compiler and -fsanitize=address,undefined and run as a child process.  Two small
// files are assembled here -- a plain RGB file with a tEXt chunk and IDAT chunks of 0, 1 and 5 bytes, and an animated file of two frames
// (acTL, an fcTL before the IDAT, an fcTL with two fdAT chunks).  Each is parsed from a heap buffer of exactly its size into span and
// frame arrays of exactly the counts and an upload buffer of exactly the data bytes, each followed by canary bytes; then cut at EVERY
// length, then with every single byte replaced by 0x00, 0xFF and a random value: each call must return TT_OK or a refusal with a text,
// without reading outside the file or writing behind the outputs.  Exit status 0 and a last line "ok" when every check held.
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

typedef std::vector<uint8_t> Bytes;
static void put32(Bytes& f, uint32_t v) { for (int s = 24; s >= 0; s -= 8) f.push_back((uint8_t)(v >> s)); }

static uint32_t crc_of(const uint8_t* p, size_t n) {
  uint32_t c = 0xffffffffu;
  for (size_t i = 0; i < n; ++i) {
    c ^= p[i];
    for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1u)));
  }
  return c ^ 0xffffffffu;
}

static void chunk(Bytes& f, const char* tag, const Bytes& body) {
  put32(f, (uint32_t)body.size());
  const size_t at = f.size();
  f.insert(f.end(), tag, tag + 4);
  f.insert(f.end(), body.begin(), body.end());
  put32(f, crc_of(f.data() + at, 4 + body.size()));
}

static Bytes head(uint32_t w, uint32_t h, int color) {
  Bytes f = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'}, b;
  put32(b, w); put32(b, h);
  b.push_back(8); b.push_back((uint8_t)color); b.push_back(0); b.push_back(0); b.push_back(0);
  chunk(f, "IHDR", b);
  return f;
}

static Bytes fctl(uint32_t seq, uint32_t w, uint32_t h) {
  Bytes b;
  put32(b, seq); put32(b, w); put32(b, h); put32(b, 0); put32(b, 0);
  b.push_back(0); b.push_back(5); b.push_back(0); b.push_back(100); b.push_back(0); b.push_back(0);
  return b;
}

static Bytes plain() {
  Bytes f = head(5, 4, 2);
  chunk(f, "tEXt", {'k', 0, 'v'});
  chunk(f, "IDAT", {});
  chunk(f, "IDAT", {0x78});
  chunk(f, "IDAT", {0x9c, 1, 2, 3, 4});
  chunk(f, "IEND", {});
  return f;
}

static Bytes animated() {
  Bytes f = head(3, 2, 0), a;
  put32(a, 2); put32(a, 7);
  chunk(f, "acTL", a);
  chunk(f, "fcTL", fctl(0, 3, 2));
  chunk(f, "IDAT", {0x78, 0x01, 9, 9});
  chunk(f, "fcTL", fctl(1, 3, 2));
  chunk(f, "fdAT", {0, 0, 0, 2, 0x78});
  chunk(f, "fdAT", {0, 0, 0, 3, 0x01, 7});
  chunk(f, "IEND", {});
  return f;
}

static const uint8_t CANARY = 0xa5;
static const size_t GUARD = 64;

static int parse_exact(const uint8_t* data, size_t n, TtPngHeader* hd, std::vector<TtPngSpan>* spans, std::vector<TtPngFrame>* frames, Bytes* upload) {
  Bytes exact(data, data + n);
  int rc = tt_png_parse(exact.data(), (int64_t)n, hd, nullptr, 0, nullptr, 0, nullptr, 0);
  if (rc != TT_OK) return rc;
  CHECK(hd->spans >= 1 && hd->frames >= 0 && hd->data_bytes >= 2 && hd->data_bytes <= (int64_t)n, "counts %d %d %lld", hd->spans, hd->frames, (long long)hd->data_bytes);
  Bytes sp((size_t)hd->spans * sizeof(TtPngSpan) + GUARD, CANARY), fr((size_t)hd->frames * sizeof(TtPngFrame) + GUARD, CANARY), up((size_t)hd->data_bytes + GUARD, CANARY);
  TtPngHeader again;
  rc = tt_png_parse(exact.data(), (int64_t)n, &again, (TtPngSpan*)sp.data(), hd->spans, (TtPngFrame*)fr.data(), hd->frames, up.data(), hd->data_bytes);
  CHECK(rc == TT_OK && again.spans == hd->spans && again.frames == hd->frames && again.data_bytes == hd->data_bytes, "the second call: rc %d %s", rc, tt_last_error());
  for (size_t i = 0; i < GUARD; ++i)
    CHECK(sp[sp.size() - GUARD + i] == CANARY && fr[fr.size() - GUARD + i] == CANARY && up[up.size() - GUARD + i] == CANARY, "a canary byte changed");
  spans->resize((size_t)hd->spans);
  memcpy(spans->data(), sp.data(), spans->size() * sizeof(TtPngSpan));
  frames->resize((size_t)hd->frames);
  if (hd->frames) memcpy(frames->data(), fr.data(), frames->size() * sizeof(TtPngFrame));
  upload->assign(up.begin(), up.end() - GUARD);
  int64_t at = 0;
  for (const TtPngSpan& s : *spans) {
    CHECK(s.bytes >= 0 && s.file_offset >= 16 && s.file_offset + s.bytes <= (int64_t)n && s.frame >= -1 && s.frame < hd->frames, "a span outside the file");
    if (rc == TT_OK && s.bytes) CHECK(memcmp(upload->data() + at, exact.data() + s.file_offset, (size_t)s.bytes) == 0, "upload is not the spans end to end");
    at += s.bytes;
  }
  CHECK(at == hd->data_bytes, "the spans do not add up");
  CHECK(hd->idat_offset >= 0 && hd->idat_offset + hd->idat_bytes <= hd->data_bytes, "the IDAT stream outside upload");
  for (const TtPngFrame& t : *frames) CHECK(t.data_offset >= 0 && t.data_bytes >= 0 && t.data_offset + t.data_bytes <= hd->data_bytes, "a frame outside upload");
  return rc;
}

static void mangle(const Bytes& file) {
  TtPngHeader hd;
  std::vector<TtPngSpan> spans;
  std::vector<TtPngFrame> frames;
  Bytes upload;
  for (size_t n = 0; n <= file.size(); ++n) {                        // cut at every length
    const int rc = parse_exact(file.data(), n, &hd, &spans, &frames, &upload);
    CHECK(rc == TT_OK || ((rc == TT_EINVAL || rc == TT_EUNSUPPORTED) && tt_last_error()[0]), "cut at %zu of %zu: rc %d", n, file.size(), rc);
  }
  for (size_t at = 0; at < file.size(); ++at)
    for (int v = 0; v < 3; ++v) {
      Bytes m = file;
      m[at] = v == 0 ? 0x00 : (v == 1 ? 0xff : (uint8_t)rnd());
      const int rc = parse_exact(m.data(), m.size(), &hd, &spans, &frames, &upload);
      CHECK(rc == TT_OK || ((rc == TT_EINVAL || rc == TT_EUNSUPPORTED) && tt_last_error()[0]), "byte %zu = %02x: rc %d", at, m[at], rc);
    }
}

int main() {
  TtPngHeader hd;
  std::vector<TtPngSpan> spans;
  std::vector<TtPngFrame> frames;
  Bytes upload;
  const Bytes a = plain(), b = animated();
  int rc = parse_exact(a.data(), a.size(), &hd, &spans, &frames, &upload);
  CHECK(rc == TT_OK, "the plain file: %d %s", rc, tt_last_error());
  CHECK(hd.width == 5 && hd.height == 4 && hd.channels == 3 && hd.bit_depth == 8 && hd.color_type == 2 && hd.interlace == 0 && hd.spans == 3 && hd.frames == 0 &&
        hd.plays == -1 && hd.default_is_frame == 0 && hd.idat_offset == 0 && hd.idat_bytes == 6 && hd.data_bytes == 6, "the plain file's header");
  const uint8_t want[6] = {0x78, 0x9c, 1, 2, 3, 4};
  CHECK(upload.size() == 6 && memcmp(upload.data(), want, 6) == 0 && spans.size() == 3 && spans[0].bytes == 0 && spans[1].bytes == 1 && spans[2].bytes == 5 &&
        spans[0].frame == -1, "the IDAT payloads, end to end");
  rc = parse_exact(b.data(), b.size(), &hd, &spans, &frames, &upload);
  CHECK(rc == TT_OK, "the animated file: %d %s", rc, tt_last_error());
  CHECK(hd.channels == 1 && hd.frames == 2 && hd.spans == 3 && hd.plays == 7 && hd.announced == 2 && hd.default_is_frame == 1 && hd.idat_bytes == 4 && hd.data_bytes == 7,
        "the animated file's header");
  if (frames.size() == 2) {
    CHECK(frames[0].sequence == 0 && frames[0].width == 3 && frames[0].height == 2 && frames[0].delay_num == 5 && frames[0].delay_den == 100 && frames[0].data_offset == 0 &&
          frames[0].data_bytes == 4 && frames[0].spans == 1, "frame 0 is the IDAT");
    CHECK(frames[1].sequence == 1 && frames[1].data_offset == 4 && frames[1].data_bytes == 3 && frames[1].spans == 2 && spans[2].frame == 1, "frame 1 is its two fdAT chunks");
    const uint8_t want2[7] = {0x78, 0x01, 9, 9, 0x78, 0x01, 7};
    CHECK(upload.size() == 7 && memcmp(upload.data(), want2, 7) == 0, "the fdAT payloads without their sequence numbers");
  }
  // the arguments
  TtPngSpan one[1];
  TtPngSpan three[3];
  uint8_t buf[16];
  CHECK(tt_png_parse(nullptr, 4, &hd, nullptr, 0, nullptr, 0, nullptr, 0) == TT_EINVAL && strstr(tt_last_error(), "null data"), "null data");
  CHECK(tt_png_parse(a.data(), (int64_t)a.size(), nullptr, nullptr, 0, nullptr, 0, nullptr, 0) == TT_EINVAL && strstr(tt_last_error(), "null header"), "null header");
  CHECK(tt_png_parse(a.data(), 0, &hd, nullptr, 0, nullptr, 0, nullptr, 0) == TT_EINVAL && strstr(tt_last_error(), "size = 0"), "size 0");
  CHECK(tt_png_parse(a.data(), (int64_t)a.size(), &hd, one, 1, nullptr, 0, nullptr, 0) == TT_EINVAL && strstr(tt_last_error(), "go together"), "one output");
  CHECK(tt_png_parse(a.data(), (int64_t)a.size(), &hd, one, 1, nullptr, 0, buf, 16) == TT_EINVAL && strstr(tt_last_error(), "span_cap too small"), "span_cap: %s", tt_last_error());
  CHECK(tt_png_parse(a.data(), (int64_t)a.size(), &hd, three, 3, nullptr, 0, buf, 5) == TT_EINVAL && strstr(tt_last_error(), "upload_cap too small"), "upload_cap: %s", tt_last_error());
  CHECK(tt_png_parse(b.data(), (int64_t)b.size(), &hd, three, 3, nullptr, 0, buf, 16) == TT_EINVAL && strstr(tt_last_error(), "frame_cap too small"), "frame_cap: %s", tt_last_error());
  mangle(a);
  mangle(b);
  if (failures) { printf("%d checks failed\n", failures); return 1; }
  printf("ok\n");
  return 0;
}
