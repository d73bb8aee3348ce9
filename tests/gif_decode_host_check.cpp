// A stand-alone program over the host routine of the GIF import (tt_gif_parse in this_and_that_vdm_amd/csrc/gif_host.cpp, with lib.cpp),
// built by tests/test_gif_decode_cpu.py with the host compiler and -fsanitize=address,undefined and run as a child process.  Two small
// files are assembled here -- a GIF89a with a global table, a NETSCAPE2.0 block, a comment, two images (the second with a local table,
// a transparent index, interlace and sub-blocks of 1, 2 and 3 bytes) and a GIF87a of one image without a trailer.  Each is parsed from
// a heap buffer of exactly its size into a frame array of exactly the count and an upload buffer of exactly the data bytes, each
// followed by canary bytes; then cut at EVERY length, then with every single byte replaced by 0x00, 0xFF and a random value: each
// call must return TT_OK or a refusal with a text, without reading outside the file or writing behind the outputs.  Exit status 0 and a
// last line "ok" when every check held.
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
static void put(Bytes& f, std::initializer_list<int> v) { for (int b : v) f.push_back((uint8_t)b); }
static void put16(Bytes& f, int v) { f.push_back((uint8_t)(v & 255)); f.push_back((uint8_t)(v >> 8)); }

static void image(Bytes& f, int left, int top, int w, int h, int flags, int colors, int mcs, const std::vector<Bytes>& blocks) {
  f.push_back(0x2c);
  put16(f, left); put16(f, top); put16(f, w); put16(f, h);
  f.push_back((uint8_t)flags);
  for (int i = 0; i < 3 * colors; ++i) f.push_back((uint8_t)(100 + i));
  f.push_back((uint8_t)mcs);
  for (const Bytes& b : blocks) { f.push_back((uint8_t)b.size()); f.insert(f.end(), b.begin(), b.end()); }
  f.push_back(0);
}

static Bytes file89() {
  Bytes f = {'G', 'I', 'F', '8', '9', 'a'};
  put16(f, 9); put16(f, 7);
  put(f, {0x80 | 0x70 | 1, 2, 0});                                  // a global table of 4 colours, background 2
  for (int i = 0; i < 12; ++i) f.push_back((uint8_t)i);
  put(f, {0x21, 0xff, 11, 'N', 'E', 'T', 'S', 'C', 'A', 'P', 'E', '2', '.', '0', 3, 1, 7, 0, 0});
  put(f, {0x21, 0xfe, 2, 'h', 'i', 0});                              // a comment
  put(f, {0x21, 0xf9, 4, (1 << 2), 10, 0, 0, 0});                    // disposal 1, delay 10
  image(f, 0, 0, 9, 7, 0, 0, 2, {{0x44, 0x01, 0x55, 0x66}});
  put(f, {0x21, 0xf9, 4, (2 << 2) | 1, 20, 0, 3, 0});                // disposal 2, transparent index 3
  image(f, 2, 1, 4, 5, 0x80 | 0x40 | 2, 8, 3, {{0x11}, {0x22, 0x33}, {0x44, 0x55, 0x66}});
  f.push_back(0x3b);
  return f;
}

static Bytes file87() {
  Bytes f = {'G', 'I', 'F', '8', '7', 'a'};
  put16(f, 3); put16(f, 2);
  put(f, {0x70, 0, 0});
  image(f, 1, 0, 2, 2, 0x80, 2, 2, {{0x84, 0x51}});
  return f;                                                          // no trailer
}

static const uint8_t CANARY = 0xa5;
static const size_t GUARD = 64;

// the two calls a caller makes, on heap copies of exactly the sizes; `frames` / `upload` come back without their canaries
static int parse_exact(const uint8_t* data, size_t n, TtGifHeader* hd, std::vector<TtGifFrame>* frames, Bytes* upload) {
  Bytes exact(data, data + n);
  int rc = tt_gif_parse(exact.data(), (int64_t)n, hd, nullptr, 0, nullptr, 0);
  if (rc != TT_OK) return rc;
  CHECK(hd->frames >= 1 && hd->data_bytes >= 0 && hd->data_bytes <= (int64_t)n, "a count of %d frames, %lld bytes", hd->frames, (long long)hd->data_bytes);
  Bytes fr((size_t)hd->frames * sizeof(TtGifFrame) + GUARD, CANARY), up((size_t)hd->data_bytes + GUARD, CANARY);
  TtGifHeader again;
  rc = tt_gif_parse(exact.data(), (int64_t)n, &again, (TtGifFrame*)fr.data(), hd->frames, up.data(), hd->data_bytes);
  CHECK(rc == TT_OK && again.frames == hd->frames && again.data_bytes == hd->data_bytes, "the second call: rc %d %s", rc, tt_last_error());
  for (size_t i = 0; i < GUARD; ++i) CHECK(fr[fr.size() - GUARD + i] == CANARY && up[up.size() - GUARD + i] == CANARY, "a canary byte changed");
  frames->resize((size_t)hd->frames);
  memcpy(frames->data(), fr.data(), frames->size() * sizeof(TtGifFrame));
  upload->assign(up.begin(), up.end() - GUARD);
  int64_t at = 0;
  for (const TtGifFrame& t : *frames) {
    CHECK(t.data_offset == at && t.data_bytes >= 0, "a frame's span %lld + %lld", (long long)t.data_offset, (long long)t.data_bytes);
    at += t.data_bytes;
    CHECK(t.w >= 1 && t.h >= 1 && t.left + t.w <= hd->width && t.top + t.h <= hd->height, "a rectangle outside the screen");
    CHECK(t.min_code_size >= 2 && t.min_code_size <= 8 && t.transparent >= -1 && t.transparent <= 255 && t.disposal >= 0 && t.disposal <= 7, "a field out of range");
  }
  CHECK(at == hd->data_bytes, "the spans do not add up");
  return rc;
}

static void mangle(const Bytes& file) {
  TtGifHeader hd;
  std::vector<TtGifFrame> frames;
  Bytes upload;
  for (size_t n = 0; n <= file.size(); ++n) {                        // cut at every length
    const int rc = parse_exact(file.data(), n, &hd, &frames, &upload);
    CHECK(rc == TT_OK || ((rc == TT_EINVAL || rc == TT_EUNSUPPORTED) && tt_last_error()[0]), "cut at %zu of %zu: rc %d", n, file.size(), rc);
  }
  for (size_t at = 0; at < file.size(); ++at)
    for (int v = 0; v < 3; ++v) {
      Bytes m = file;
      m[at] = v == 0 ? 0x00 : (v == 1 ? 0xff : (uint8_t)rnd());
      const int rc = parse_exact(m.data(), m.size(), &hd, &frames, &upload);
      CHECK(rc == TT_OK || ((rc == TT_EINVAL || rc == TT_EUNSUPPORTED) && tt_last_error()[0]), "byte %zu = %02x: rc %d", at, m[at], rc);
    }
}

int main() {
  TtGifHeader hd;
  std::vector<TtGifFrame> frames;
  Bytes upload;
  const Bytes a = file89(), b = file87();
  int rc = parse_exact(a.data(), a.size(), &hd, &frames, &upload);
  CHECK(rc == TT_OK, "the GIF89a file: %d %s", rc, tt_last_error());
  CHECK(hd.width == 9 && hd.height == 7 && hd.background == 2 && hd.loop == 7 && hd.global_colors == 4 && hd.frames == 2 && hd.version == 89 && hd.data_bytes == 10,
        "header %d %d %d %d %d %d %d %lld", hd.width, hd.height, hd.background, hd.loop, hd.global_colors, hd.frames, hd.version, (long long)hd.data_bytes);
  if (frames.size() == 2) {
    const TtGifFrame &f0 = frames[0], &f1 = frames[1];
    CHECK(f0.left == 0 && f0.w == 9 && f0.h == 7 && !f0.interlace && f0.transparent == -1 && f0.disposal == 1 && f0.delay == 10 && f0.min_code_size == 2 &&
          f0.local_colors == 0 && f0.data_bytes == 4, "frame 0");
    CHECK(f0.palette[3][2] == 11 && f0.palette[4][0] == 0 && f0.palette[255][2] == 0, "frame 0's palette is the global table, zero-padded");
    CHECK(f1.left == 2 && f1.top == 1 && f1.w == 4 && f1.h == 5 && f1.interlace == 1 && f1.transparent == 3 && f1.disposal == 2 && f1.delay == 20 &&
          f1.min_code_size == 3 && f1.local_colors == 8 && f1.data_offset == 4 && f1.data_bytes == 6, "frame 1");
    CHECK(f1.palette[0][0] == 100 && f1.palette[7][2] == 123 && f1.palette[8][0] == 0, "frame 1's palette is its local table, zero-padded");
    const uint8_t want[10] = {0x44, 0x01, 0x55, 0x66, 0x11, 0x22, 0x33, 0x44, 0x55, 0x66};
    CHECK(upload.size() == 10 && memcmp(upload.data(), want, 10) == 0, "the sub-blocks' payload, end to end");
  }
  rc = parse_exact(b.data(), b.size(), &hd, &frames, &upload);
  CHECK(rc == TT_OK && hd.version == 87 && hd.loop == -1 && hd.global_colors == 0 && hd.frames == 1 && frames[0].local_colors == 2 && frames[0].transparent == -1 &&
        frames[0].disposal == 0 && frames[0].delay == 0, "the GIF87a file without a trailer: %d %s", rc, tt_last_error());
  // the arguments
  TtGifFrame one[1];
  uint8_t buf[16];
  CHECK(tt_gif_parse(nullptr, 4, &hd, nullptr, 0, nullptr, 0) == TT_EINVAL && strstr(tt_last_error(), "null data"), "null data");
  CHECK(tt_gif_parse(a.data(), (int64_t)a.size(), nullptr, nullptr, 0, nullptr, 0) == TT_EINVAL && strstr(tt_last_error(), "null header"), "null header");
  CHECK(tt_gif_parse(a.data(), 0, &hd, nullptr, 0, nullptr, 0) == TT_EINVAL && strstr(tt_last_error(), "size = 0"), "size 0");
  CHECK(tt_gif_parse(a.data(), (int64_t)a.size(), &hd, one, 1, nullptr, 0) == TT_EINVAL && strstr(tt_last_error(), "go together"), "one output");
  CHECK(tt_gif_parse(a.data(), (int64_t)a.size(), &hd, one, 1, buf, 16) == TT_EINVAL && strstr(tt_last_error(), "frame_cap too small"), "frame_cap: %s", tt_last_error());
  TtGifFrame two[2];
  CHECK(tt_gif_parse(a.data(), (int64_t)a.size(), &hd, two, 2, buf, 9) == TT_EINVAL && strstr(tt_last_error(), "upload_cap too small"), "upload_cap: %s", tt_last_error());
  mangle(a);
  mangle(b);
  if (failures) { printf("%d checks failed\n", failures); return 1; }
  printf("ok\n");
  return 0;
}
