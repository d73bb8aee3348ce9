// A stand-alone program over the host half of the GIF export (this_and_that_vdm_amd/csrc/gif_host.cpp + lib.cpp), built by
// tests/test_gif_export_cpu.py with the host compiler and -fsanitize=address,undefined and run as a child process: the median-cut
// cases with their invariants, and tt_gif_lzw on random, constant and 1 x 1 inputs with an in-program decode compared to the input.
// Exit status 0 and a last line "ok" when every check held.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
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

// `bins` occupied bins (all of them when bins == TT_GIF_BINS), each with 1 .. maxcount pixels whose channels lie inside the bin
static std::vector<TtColorBin> make_hist(int bins, uint32_t maxcount) {
  std::vector<TtColorBin> h(TT_GIF_BINS);
  memset(h.data(), 0, h.size() * sizeof(TtColorBin));
  int made = 0;
  while (made < bins) {
    const int bin = bins == TT_GIF_BINS ? made : (int)(rnd() % TT_GIF_BINS);
    if (h[bin].count) continue;
    const uint32_t n = 1 + rnd() % maxcount;
    h[bin].count = n;
    for (uint32_t i = 0; i < n; ++i) {
      h[bin].sum_r += (uint32_t)((bin >> 10) << 3) + rnd() % 8;
      h[bin].sum_g += (uint32_t)(((bin >> 5) & 31) << 3) + rnd() % 8;
      h[bin].sum_b += (uint32_t)((bin & 31) << 3) + rnd() % 8;
    }
    ++made;
  }
  return h;
}

static void median_cut_case(int bins, int colors, uint32_t maxcount) {
  const std::vector<TtColorBin> h = make_hist(bins, maxcount);
  uint8_t pal[256 * 3];
  int32_t n = -1;
  std::vector<int32_t> box(TT_GIF_BINS);
  const int rc = tt_palette_median_cut(h.data(), colors, pal, &n, box.data());
  CHECK(rc == TT_OK, "median cut (%d bins, %d colors): %d %s", bins, colors, rc, tt_last_error());
  if (rc != TT_OK) return;
  CHECK(n == (bins < colors ? bins : colors), "median cut (%d bins, %d colors): %d entries", bins, colors, n);
  int lo[256][3], hi[256][3], members[256];
  for (int k = 0; k < 256; ++k) { members[k] = 0; for (int c = 0; c < 3; ++c) { lo[k][c] = 255; hi[k][c] = 0; } }
  for (int bin = 0; bin < TT_GIF_BINS; ++bin) {
    if (!h[bin].count) { CHECK(box[bin] == -1, "empty bin %d in box %d", bin, box[bin]); continue; }
    const int k = box[bin];
    CHECK(k >= 0 && k < n, "bin %d in box %d of %d", bin, k, n);
    if (k < 0 || k >= n) continue;
    ++members[k];
    const int c3[3] = {(bin >> 10) << 3, ((bin >> 5) & 31) << 3, (bin & 31) << 3};
    for (int c = 0; c < 3; ++c) {
      if (c3[c] < lo[k][c]) lo[k][c] = c3[c];
      if (c3[c] + 7 > hi[k][c]) hi[k][c] = c3[c] + 7;
    }
  }
  for (int k = 0; k < n; ++k) {
    CHECK(members[k] > 0, "box %d is empty", k);
    for (int c = 0; c < 3; ++c) CHECK(pal[3 * k + c] >= lo[k][c] && pal[3 * k + c] <= hi[k][c], "entry %d channel %d = %d outside [%d, %d]", k, c, pal[3 * k + c], lo[k][c], hi[k][c]);
  }
  for (int i = 3 * n; i < 768; ++i) CHECK(pal[i] == 0, "palette byte %d behind the last entry is %d", i, pal[i]);
}

// the textbook decoder of GIF89a appendix F over the sub-blocks tt_gif_lzw wrote
static bool lzw_decode(const std::vector<uint8_t>& data, std::vector<uint8_t>& out) {
  std::vector<uint8_t> payload;
  size_t pos = 1;
  while (pos < data.size() && data[pos]) {
    if (pos + 1 + data[pos] > data.size()) return false;
    payload.insert(payload.end(), data.begin() + pos + 1, data.begin() + pos + 1 + data[pos]);
    pos += 1 + (size_t)data[pos];
  }
  if (pos + 1 != data.size()) return false;          // the terminator is the last byte
  const int mcs = data[0], clear = 1 << mcs, eoi = clear + 1;
  std::vector<int> prefix(4096, -1);
  std::vector<uint8_t> last(4096, 0), first(4096, 0);
  int width = mcs + 1, next = eoi + 1, prev = -1;
  size_t at = 0;
  std::vector<uint8_t> run;
  for (;;) {
    if (at + width > 8 * payload.size()) return false;
    int code = 0;
    for (int b = 0; b < width; ++b, ++at) code |= ((payload[at >> 3] >> (at & 7)) & 1) << b;
    if (code == clear) { width = mcs + 1; next = eoi + 1; prev = -1; continue; }
    if (code == eoi) return 8 * payload.size() - at < 8;
    int entry = code;
    if (prev >= 0) {
      if (code > next || (code == next && next >= 4096)) return false;
      if (next < 4096) {
        prefix[next] = prev;
        first[next] = prev < clear ? (uint8_t)prev : first[prev];
        const int head = code == next ? prev : code;
        last[next] = head < clear ? (uint8_t)head : first[head];
        ++next;
        if (next == (1 << width) && width < 12) ++width;
      }
    } else if (code >= clear) return false;
    run.clear();
    for (int e = entry; e >= 0; e = e < clear ? -1 : prefix[e]) run.push_back(e < clear ? (uint8_t)e : last[e]);
    out.insert(out.end(), run.rbegin(), run.rend());
    prev = entry;
  }
}

static void lzw_case(const char* name, const std::vector<uint8_t>& idx, int mcs) {
  const int64_t cap = tt_gif_lzw_bound((int64_t)idx.size());
  std::vector<uint8_t> out((size_t)cap);            // exactly the bound: a byte beyond it is the sanitizer's to report
  int64_t n = -1;
  const int rc = tt_gif_lzw(idx.data(), (int64_t)idx.size(), mcs, out.data(), cap, &n);
  CHECK(rc == TT_OK && n > 0 && n <= cap, "lzw %s: %d %s (n = %lld, cap = %lld)", name, rc, tt_last_error(), (long long)n, (long long)cap);
  if (rc != TT_OK) return;
  out.resize((size_t)n);
  std::vector<uint8_t> back;
  CHECK(lzw_decode(out, back), "lzw %s: the stream does not decode", name);
  CHECK(back == idx, "lzw %s: %zu indices decoded from %zu, or other values", name, back.size(), idx.size());
  for (int64_t small : {(int64_t)0, (int64_t)1, n / 2, n - 1}) {                 // too small a buffer is an error and never an overrun
    std::vector<uint8_t> tight((size_t)(small > 0 ? small : 1));
    int64_t m = -1;
    CHECK(tt_gif_lzw(idx.data(), (int64_t)idx.size(), mcs, tight.data(), small, &m) == TT_EINVAL, "lzw %s: cap %lld accepted", name, (long long)small);
  }
}

int main() {
  median_cut_case(5000, 256, 40);
  median_cut_case(TT_GIF_BINS, 256, 3);
  median_cut_case(256, 256, 5);
  median_cut_case(257, 256, 5);
  median_cut_case(1, 256, 9);
  median_cut_case(5000, 2, 40);
  median_cut_case(5000, 16, 40);
  median_cut_case(4000, 256, 1);                     // every count 1: ties everywhere
  std::vector<uint8_t> idx(96 * 96);
  for (auto& v : idx) v = (uint8_t)(rnd() & 255);
  lzw_case("random 96 x 96", idx, 8);
  lzw_case("constant 300 x 200", std::vector<uint8_t>(300 * 200, 7), 8);
  lzw_case("1 x 1", std::vector<uint8_t>(1, 3), 2);
  for (auto& v : idx) v &= 1;
  lzw_case("two colours", idx, 2);
  for (int mcs = 2; mcs <= 8; ++mcs) {               // lengths around the points where the width grows just before the end
    for (int len = 1; len <= 40; ++len) {
      std::vector<uint8_t> v((size_t)len);
      for (auto& x : v) x = (uint8_t)(rnd() % (1u << mcs));
      lzw_case("short", v, mcs);
    }
  }
  uint8_t pal[768];
  int32_t n = 0;
  std::vector<TtColorBin> empty(TT_GIF_BINS);
  memset(empty.data(), 0, empty.size() * sizeof(TtColorBin));
  CHECK(tt_palette_median_cut(empty.data(), 256, pal, &n, NULL) == TT_EINVAL, "an empty histogram was accepted");
  CHECK(tt_palette_median_cut(empty.data(), 0, pal, &n, NULL) == TT_EINVAL, "colors = 0 was accepted");
  if (failures) { printf("%d checks failed\n", failures); return 1; }
  printf("ok\n");
  return 0;
}
