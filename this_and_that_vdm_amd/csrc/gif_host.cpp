// libttvdm: the host half of the GIF export -- tt_palette_median_cut (a median cut over the occupied bins of one colour histogram) and
// tt_gif_lzw (the image data of one GIF frame).  include/ttvdm.h states both rule by rule; integers only.
#include "gif_host.h"

#include <string.h>
#include <vector>

namespace {

struct Box {
  std::vector<int> bins;                            // occupied bins, in ascending bin order
  uint64_t count = 0;                               // pixels
};

inline int coord(int bin, int axis) { return (bin >> (10 - 5 * axis)) & 31; }      // axis 0 R, 1 G, 2 B

// rules 2 - 5 of the header: box `b` keeps the lower part, the rest goes to `upper`
void split(const TtColorBin* hist, Box& b, Box& upper) {
  int lo[3] = {31, 31, 31}, hi[3] = {0, 0, 0};
  for (int bin : b.bins)
    for (int a = 0; a < 3; ++a) {
      const int c = coord(bin, a);
      if (c < lo[a]) lo[a] = c;
      if (c > hi[a]) hi[a] = c;
    }
  int axis = 0;
  for (int a = 1; a < 3; ++a)
    if (hi[a] - lo[a] > hi[axis] - lo[axis]) axis = a;            // strictly larger: ties stay with R, then G
  uint64_t at[32] = {0};
  for (int bin : b.bins) at[coord(bin, axis)] += hist[bin].count;
  int t = lo[axis];
  for (uint64_t run = 0;; ++t) {
    run += at[t];
    if (2 * run >= b.count) break;
  }
  if (t == hi[axis])
    for (--t; at[t] == 0; --t) {}                                  // the box holds two coordinates at least: lo[axis] ends this
  std::vector<int> keep;
  uint64_t kept = 0;
  for (int bin : b.bins) {
    if (coord(bin, axis) <= t) { keep.push_back(bin); kept += hist[bin].count; }
    else upper.bins.push_back(bin);
  }
  upper.count = b.count - kept;
  b.bins.swap(keep);
  b.count = kept;
}

// ---- LZW: the output side (codes packed from the least significant bit into sub-blocks of at most 255 bytes) ...
struct BitSink {
  uint8_t* out;
  int64_t cap, pos, block;                          // block: where the open sub-block's length byte is; -1 when none is open
  uint32_t acc = 0;
  int nacc = 0;
  bool full = false;
  BitSink(uint8_t* o, int64_t c) : out(o), cap(c), pos(0), block(-1) {}
  void raw(uint8_t v) {
    if (pos < cap) out[pos++] = v;
    else full = true;
  }
  void data(uint8_t v) {
    if (block < 0) { block = pos; raw(0); }
    raw(v);
    if (!full && ++out[block] == 255) block = -1;
  }
  void code(uint32_t c, int width) {
    acc |= c << nacc;
    nacc += width;
    for (; nacc >= 8; nacc -= 8, acc >>= 8) data((uint8_t)(acc & 0xffu));
  }
  void finish() {
    if (nacc > 0) data((uint8_t)(acc & 0xffu));
    nacc = 0;
    block = -1;
    raw(0);                                         // the block terminator
  }
};

// ... and the string table: (prefix code, next index) -> code, open addressing over twice the table's entries
struct Strings {
  static constexpr int SIZE = 2 * TT_LZW_MAX_CODES;
  static constexpr uint32_t NONE = 0xffffffffu;
  uint32_t key[SIZE];
  uint16_t val[SIZE];
  void clear() { memset(key, 0xff, sizeof key); }
  static int slot_of(uint32_t k) { return (int)((k * 0x9E3779B1u) >> (32 - 13)); }
  int find(uint32_t k, int* where) const {
    int s = slot_of(k);
    for (; key[s] != NONE; s = (s + 1) & (SIZE - 1))
      if (key[s] == k) return val[s];
    *where = s;
    return -1;
  }
};
static_assert(Strings::SIZE == 1 << 13, "slot_of keeps 13 bits");

}  // namespace

extern "C" int tt_palette_median_cut(const TtColorBin* hist, int32_t colors, uint8_t* palette, int32_t* ncolors_out, int32_t* bin_box) {
  if (!hist || !palette || !ncolors_out) TT_FAIL(TT_EINVAL, "tt_palette_median_cut: null %s", !hist ? "hist" : (!palette ? "palette" : "ncolors_out"));
  if (colors < 1 || colors > 256) TT_FAIL(TT_EINVAL, "tt_palette_median_cut: colors = %d (1 to 256)", colors);
  std::vector<Box> boxes(1);
  boxes.reserve((size_t)colors);
  for (int bin = 0; bin < TT_GIF_BINS; ++bin)
    if (hist[bin].count) { boxes[0].bins.push_back(bin); boxes[0].count += hist[bin].count; }
  if (boxes[0].bins.empty()) TT_FAIL(TT_EINVAL, "tt_palette_median_cut: the histogram holds no pixel");
  while ((int)boxes.size() < colors) {
    int pick = -1;
    for (int i = 0; i < (int)boxes.size(); ++i)
      if (boxes[i].bins.size() > 1 && (pick < 0 || boxes[i].count > boxes[pick].count)) pick = i;      // strictly larger: the earliest keeps a tie
    if (pick < 0) break;
    Box upper;
    split(hist, boxes[pick], upper);
    boxes.push_back(std::move(upper));
  }
  memset(palette, 0, 256 * 3);
  if (bin_box)
    for (int bin = 0; bin < TT_GIF_BINS; ++bin) bin_box[bin] = -1;
  for (int k = 0; k < (int)boxes.size(); ++k) {
    uint64_t s[3] = {0, 0, 0};
    for (int bin : boxes[k].bins) {
      s[0] += hist[bin].sum_r;
      s[1] += hist[bin].sum_g;
      s[2] += hist[bin].sum_b;
      if (bin_box) bin_box[bin] = k;
    }
    for (int c = 0; c < 3; ++c) {
      const uint64_t v = (2 * s[c] + boxes[k].count) / (2 * boxes[k].count);
      palette[3 * k + c] = (uint8_t)(v > 255 ? 255 : v);           // (a consistent histogram never exceeds 255)
    }
  }
  *ncolors_out = (int32_t)boxes.size();
  return TT_OK;
}

extern "C" int64_t tt_gif_lzw_bound(int64_t npix) {
  if (npix <= 0) return 0;
  const int64_t codes = npix + npix / 2048 + 4;                    // one per index at most, the clear codes, the first clear and the end
  const int64_t data = (codes * TT_LZW_MAX_BITS + 7) / 8;
  return 1 + data + (data + 254) / 255 + 1;                        // the min-code-size byte, data, one length byte per sub-block, terminator
}

extern "C" int tt_gif_lzw(const uint8_t* indices, int64_t npix, int32_t min_code_size, uint8_t* out, int64_t cap, int64_t* nbytes_out) {
  if (!indices || !out || !nbytes_out) TT_FAIL(TT_EINVAL, "tt_gif_lzw: null %s", !indices ? "indices" : (!out ? "out" : "nbytes_out"));
  if (npix <= 0) TT_FAIL(TT_EINVAL, "tt_gif_lzw: npix = %lld", (long long)npix);
  if (min_code_size < 2 || min_code_size > 8) TT_FAIL(TT_EINVAL, "tt_gif_lzw: min_code_size = %d (2 to 8)", min_code_size);
  const uint32_t clear = 1u << min_code_size, eoi = clear + 1;
  std::vector<Strings> table(1);
  Strings& tab = table[0];
  tab.clear();
  BitSink sink(out, cap);
  sink.raw((uint8_t)min_code_size);
  int width = min_code_size + 1;
  uint32_t next = eoi + 1;
  sink.code(clear, width);
  if (indices[0] >= clear) TT_FAIL(TT_EINVAL, "tt_gif_lzw: index %d at 0 does not fit min_code_size %d", indices[0], min_code_size);
  uint32_t prefix = indices[0];
  for (int64_t i = 1; i < npix && !sink.full; ++i) {
    const uint32_t c = indices[i];
    if (c >= clear) TT_FAIL(TT_EINVAL, "tt_gif_lzw: index %u at %lld does not fit min_code_size %d", c, (long long)i, min_code_size);
    const uint32_t k = (prefix << 8) | c;
    int where = 0;
    const int found = tab.find(k, &where);
    if (found >= 0) { prefix = (uint32_t)found; continue; }
    sink.code(prefix, width);
    if (next < (uint32_t)TT_LZW_MAX_CODES) {
      tab.key[where] = k;
      tab.val[where] = (uint16_t)next;
      if (next == (1u << width) && width < TT_LZW_MAX_BITS) ++width;
      ++next;
    } else {
      sink.code(clear, width);
      tab.clear();
      width = min_code_size + 1;
      next = eoi + 1;
    }
    prefix = c;
  }
  sink.code(prefix, width);
  if (next == (1u << width) && width < TT_LZW_MAX_BITS) ++width;   // a decoder makes its entry `next` on reading that code, and widens with it
  sink.code(eoi, width);
  sink.finish();
  if (sink.full) TT_FAIL(TT_EINVAL, "tt_gif_lzw: cap = %lld bytes is too small (tt_gif_lzw_bound: %lld)", (long long)cap, (long long)tt_gif_lzw_bound(npix));
  *nbytes_out = sink.pos;
  return TT_OK;
}
