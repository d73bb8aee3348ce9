// libttvdm: the host half of the GIF export -- tt_palette_median_cut (a median cut over the occupied bins of one colour histogram) and
// tt_gif_lzw (the image data of one GIF frame) -- and of the GIF import: tt_gif_parse (the container).  include/ttvdm.h states all three
// rule by rule; integers only.
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

// ---- the GIF import's container (include/ttvdm.h, "GIF import", rule 1).  `at` only ever grows, so every loop ends with the file.
namespace {

struct Reader {
  const uint8_t* p;
  int64_t size, at = 0;
  bool has(int64_t n) const { return n >= 0 && n <= size - at; }
  uint8_t u8() { return p[at++]; }
  int u16() { const int v = p[at] | (p[at + 1] << 8); at += 2; return v; }
};

// skips a chain of sub-blocks behind `r.at`; false when the file ends inside it
bool skip_blocks(Reader& r) {
  for (;;) {
    if (!r.has(1)) return false;
    const int n = r.u8();
    if (n == 0) return true;
    if (!r.has(n)) return false;
    r.at += n;
  }
}

}  // namespace

extern "C" int tt_gif_parse(const uint8_t* data, int64_t size, TtGifHeader* header, TtGifFrame* frames, int64_t frame_cap, uint8_t* upload,
                            int64_t upload_cap) {
  if (!data || !header) TT_FAIL(TT_EINVAL, "tt_gif_parse: null %s", !data ? "data" : "header");
  if (size <= 0) TT_FAIL(TT_EINVAL, "tt_gif_parse: size = %lld", (long long)size);
  if ((frames == nullptr) != (upload == nullptr)) TT_FAIL(TT_EINVAL, "tt_gif_parse: frames and upload go together (both, or neither to count)");
  if (frames && (frame_cap < 0 || upload_cap < 0)) TT_FAIL(TT_EINVAL, "tt_gif_parse: frame_cap = %lld, upload_cap = %lld", (long long)frame_cap, (long long)upload_cap);
  Reader r{data, size};
  if (!r.has(6)) TT_FAIL(TT_EINVAL, "tt_gif_parse: the file ends inside the signature (%lld bytes)", (long long)size);
  if (memcmp(data, "GIF87a", 6) != 0 && memcmp(data, "GIF89a", 6) != 0) TT_FAIL(TT_EINVAL, "tt_gif_parse: bad signature (neither GIF87a nor GIF89a)");
  r.at = 6;
  TtGifHeader hd = {};
  hd.version = data[4] == '7' ? 87 : 89;
  hd.loop = -1;
  if (!r.has(7)) TT_FAIL(TT_EINVAL, "tt_gif_parse: the file ends inside the logical screen descriptor");
  hd.width = r.u16();
  hd.height = r.u16();
  const int packed = r.u8();
  hd.background = r.u8();
  r.u8();                                                          // the pixel aspect ratio
  uint8_t global[256][3];
  memset(global, 0, sizeof global);
  if (packed & 0x80) {
    hd.global_colors = 2 << (packed & 7);
    if (!r.has(3 * hd.global_colors)) TT_FAIL(TT_EINVAL, "tt_gif_parse: the file ends inside the global colour table");
    memcpy(global, data + r.at, (size_t)(3 * hd.global_colors));
    r.at += 3 * hd.global_colors;
  }
  if ((int64_t)hd.width * hd.height > TT_GIF_MAX_PIXELS)
    TT_FAIL(TT_EUNSUPPORTED, "tt_gif_parse: a canvas of %d x %d pixels (at most TT_GIF_MAX_PIXELS = %d)", hd.width, hd.height, TT_GIF_MAX_PIXELS);
  int transparent = -1, disposal = 0, delay = 0;                    // of the graphic control extension before the next image
  int64_t nframes = 0, nbytes = 0;
  while (r.has(1)) {
    const int block = r.u8();
    if (block == 0x3b) break;                                       // the trailer
    if (block == 0x21) {
      if (!r.has(1)) TT_FAIL(TT_EINVAL, "tt_gif_parse: the file ends inside an extension (before frame %lld)", (long long)nframes);
      const int label = r.u8();
      if (label == 0xf9 && r.has(6) && data[r.at] == 4) {           // graphic control: size 4, packed, delay, transparent index
        const int gp = data[r.at + 1];
        disposal = (gp >> 2) & 7;
        delay = data[r.at + 2] | (data[r.at + 3] << 8);
        transparent = (gp & 1) ? data[r.at + 4] : -1;
      } else if (label == 0xff && r.has(17) && data[r.at] == 11 && memcmp(data + r.at + 1, "NETSCAPE2.0", 11) == 0 && data[r.at + 12] == 3 &&
                 data[r.at + 13] == 1) {
        hd.loop = data[r.at + 14] | (data[r.at + 15] << 8);
      }
      if (!skip_blocks(r)) TT_FAIL(TT_EINVAL, "tt_gif_parse: the file ends inside an extension's sub-block (before frame %lld)", (long long)nframes);
      continue;
    }
    if (block != 0x2c) {
      if (nframes > 0) break;                                       // bytes behind a complete image: taken as a missing trailer
      TT_FAIL(TT_EINVAL, "tt_gif_parse: unknown block 0x%02x at byte %lld", block, (long long)(r.at - 1));
    }
    const long long f = (long long)nframes;
    if (nframes >= TT_GIF_MAX_FRAMES) TT_FAIL(TT_EUNSUPPORTED, "tt_gif_parse: more than %d frames", TT_GIF_MAX_FRAMES);
    if (!r.has(9)) TT_FAIL(TT_EINVAL, "tt_gif_parse: the file ends inside the image descriptor of frame %lld", f);
    TtGifFrame fr = {};
    fr.left = r.u16();
    fr.top = r.u16();
    fr.w = r.u16();
    fr.h = r.u16();
    const int ip = r.u8();
    fr.interlace = (ip >> 6) & 1;
    fr.transparent = transparent;
    fr.disposal = disposal;
    fr.delay = delay;
    transparent = -1, disposal = 0, delay = 0;
    if (fr.w == 0 || fr.h == 0) TT_FAIL(TT_EINVAL, "tt_gif_parse: frame %lld has a rectangle of zero size (%d x %d)", f, fr.w, fr.h);
    if (fr.left + fr.w > hd.width || fr.top + fr.h > hd.height)
      TT_FAIL(TT_EINVAL, "tt_gif_parse: frame %lld's rectangle (%d, %d, %d x %d) leaves the logical screen of %d x %d", f, fr.left, fr.top, fr.w, fr.h, hd.width,
              hd.height);
    const uint8_t* table = &global[0][0];
    int colors = hd.global_colors;
    if (ip & 0x80) {
      fr.local_colors = colors = 2 << (ip & 7);
      if (!r.has(3 * colors)) TT_FAIL(TT_EINVAL, "tt_gif_parse: the file ends inside the local colour table of frame %lld", f);
      table = data + r.at;
      r.at += 3 * colors;
    }
    if (colors == 0) TT_FAIL(TT_EINVAL, "tt_gif_parse: frame %lld has no colour table, neither a local nor a global one", f);
    if (!r.has(1)) TT_FAIL(TT_EINVAL, "tt_gif_parse: the file ends inside the image data of frame %lld", f);
    fr.min_code_size = r.u8();
    if (fr.min_code_size < 2 || fr.min_code_size > 8) TT_FAIL(TT_EINVAL, "tt_gif_parse: frame %lld has a minimum code size of %d (2 to 8)", f, fr.min_code_size);
    fr.data_offset = nbytes;
    for (;;) {
      if (!r.has(1)) TT_FAIL(TT_EINVAL, "tt_gif_parse: the file ends inside the image data of frame %lld (no block terminator)", f);
      const int n = r.u8();
      if (n == 0) break;
      if (!r.has(n)) TT_FAIL(TT_EINVAL, "tt_gif_parse: the file ends inside a sub-block of frame %lld", f);
      if (upload) {
        if (nbytes + n > upload_cap) TT_FAIL(TT_EINVAL, "tt_gif_parse: upload_cap too small: %lld bytes", (long long)upload_cap);
        memcpy(upload + nbytes, data + r.at, (size_t)n);
      }
      nbytes += n;
      r.at += n;
    }
    fr.data_bytes = nbytes - fr.data_offset;
    if (fr.data_bytes >= (1ll << 29)) TT_FAIL(TT_EUNSUPPORTED, "tt_gif_parse: frame %lld has %lld data bytes (fewer than 2^29 = 536870912)", f, (long long)fr.data_bytes);
    if (frames) {
      if (nframes >= frame_cap) TT_FAIL(TT_EINVAL, "tt_gif_parse: frame_cap too small: %lld", (long long)frame_cap);
      memcpy(fr.palette, table, (size_t)(3 * colors));              // the rest of the 256 entries stays zero
      frames[nframes] = fr;
    }
    ++nframes;
  }
  if (nframes == 0) TT_FAIL(TT_EINVAL, "tt_gif_parse: no image at all in %lld bytes", (long long)size);
  hd.frames = (int32_t)nframes;
  hd.data_bytes = nbytes;
  *header = hd;
  return TT_OK;
}
