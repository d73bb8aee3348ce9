// libttvdm: the host half of the PNG export -- tt_png_code_lengths (length-limited Huffman code lengths by package-merge),
// tt_png_block_header (the dynamic-block header of one stripe and the stripe's exact size) and tt_png_plan (both for every stripe of a
// call, with the code tables and byte offsets tt_png_emit reads).  include/ttvdm.h states them rule by rule; integers only.
#include "png_host.h"

#include "huffman_host.h"

#include <stdio.h>
#include <string.h>
#include <vector>

namespace {

// canonical codes (RFC 1951 3.2.2) with their bits reversed: ready to be ORed in from the least significant bit
void reversed_codes(const uint8_t* lengths, int nsym, uint32_t* codes) {
  int per[16] = {0};
  for (int s = 0; s < nsym; ++s) ++per[lengths[s]];
  per[0] = 0;
  uint32_t next[16] = {0}, code = 0;
  for (int b = 1; b <= 15; ++b) { code = (code + (uint32_t)per[b - 1]) << 1; next[b] = code; }
  for (int s = 0; s < nsym; ++s) {
    uint32_t c = lengths[s] ? next[lengths[s]]++ : 0, r = 0;
    for (int b = 0; b < lengths[s]; ++b, c >>= 1) r = (r << 1) | (c & 1u);
    codes[s] = r;
  }
}

struct BitSink {                                   // bits from the least significant bit of each word; at most 16 per put
  uint32_t* words;
  int cap_bits, n = 0;
  bool full = false;
  BitSink(uint32_t* w, int cap_words) : words(w), cap_bits(cap_words * 32) { memset(w, 0, (size_t)cap_words * 4); }
  void put(uint32_t v, int k) {
    if (n + k > cap_bits) { full = true; return; }
    const int word = n >> 5, sh = n & 31;
    words[word] |= v << sh;
    if (sh + k > 32) words[word + 1] |= v >> (32 - sh);
    n += k;
  }
};

struct ClToken { uint8_t sym, extra_bits, extra; };

// rule 5's greedy run coding of the HLIT + 257 literal/length lengths and the one distance length
void run_code(const std::vector<uint8_t>& seq, std::vector<ClToken>& out) {
  for (size_t i = 0; i < seq.size();) {
    const uint8_t v = seq[i];
    size_t run = 1;
    while (i + run < seq.size() && seq[i + run] == v) ++run;
    i += run;
    if (v == 0) {
      while (run >= 11) { const size_t t = run < 138 ? run : 138; out.push_back({18, 7, (uint8_t)(t - 11)}); run -= t; }
      if (run >= 3) { out.push_back({17, 3, (uint8_t)(run - 3)}); run = 0; }
    } else {
      out.push_back({v, 0, 0});
      --run;
      while (run >= 3) { const size_t t = run < 6 ? run : 6; out.push_back({16, 2, (uint8_t)(t - 3)}); run -= t; }
    }
    for (; run > 0; --run) out.push_back({v, 0, 0});
  }
}

const uint8_t CL_ORDER[TT_PNG_CL_SYMS] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

int block_header(const char* who, const uint32_t* counts, const uint8_t* lengths, uint32_t* header, int32_t cap_words, int64_t* stripe_bits_out) {
  if (cap_words < TT_PNG_HEADER_WORDS) TT_FAIL(TT_EINVAL, "%s: cap too small: %d words, a header takes up to %d (TT_PNG_HEADER_WORDS)", who, cap_words, TT_PNG_HEADER_WORDS);
  uint64_t kraft = 0;
  int last = 256;
  int64_t data_bits = 0;
  for (int s = 0; s < TT_PNG_SYMS; ++s) {
    if (lengths[s] > TT_PNG_LIT_LIMIT) TT_FAIL(TT_EINVAL, "%s: lengths[%d] = %d (at most %d)", who, s, lengths[s], TT_PNG_LIT_LIMIT);
    if ((counts[s] || s == 256) && !lengths[s]) TT_FAIL(TT_EINVAL, "%s: symbol %d is used and has no length", who, s);
    if (lengths[s]) { kraft += 1ull << (TT_PNG_LIT_LIMIT - lengths[s]); if (s > last) last = s; }
    data_bits += (int64_t)counts[s] * (lengths[s] + (s > 256 ? tt_png_length_extra(s) + 1 : 0));      // + 1: the match's distance bit
  }
  if (kraft > (1ull << TT_PNG_LIT_LIMIT)) TT_FAIL(TT_EINVAL, "%s: the lengths' Kraft sum exceeds 1", who);
  const int hlit = last + 1;
  std::vector<uint8_t> seq(lengths, lengths + hlit);
  seq.push_back(1);
  std::vector<ClToken> toks;
  run_code(seq, toks);
  uint32_t cl_counts[TT_PNG_CL_SYMS] = {0}, cl_codes[TT_PNG_CL_SYMS];
  uint8_t cl_len[TT_PNG_CL_SYMS];
  for (const ClToken& t : toks) ++cl_counts[t.sym];
  const int rc = tt_code_lengths(who, cl_counts, TT_PNG_CL_SYMS, TT_PNG_CL_LIMIT, cl_len);
  if (rc != TT_OK) return rc;
  reversed_codes(cl_len, TT_PNG_CL_SYMS, cl_codes);
  int hclen = 4;
  for (int i = 4; i < TT_PNG_CL_SYMS; ++i)
    if (cl_len[CL_ORDER[i]]) hclen = i + 1;
  BitSink sink(header + 1, cap_words - 1);
  sink.put(0, 1);                                   // BFINAL
  sink.put(2, 2);                                   // BTYPE: dynamic codes
  sink.put((uint32_t)(hlit - 257), 5);
  sink.put(0, 5);                                   // HDIST - 1: one distance code
  sink.put((uint32_t)(hclen - 4), 4);
  for (int i = 0; i < hclen; ++i) sink.put(cl_len[CL_ORDER[i]], 3);
  for (const ClToken& t : toks) {
    sink.put(cl_codes[t.sym], cl_len[t.sym]);
    if (t.extra_bits) sink.put(t.extra, t.extra_bits);
  }
  if (sink.full) TT_FAIL(TT_EINVAL, "%s: cap too small: the header does not fit %d words", who, cap_words);
  header[0] = (uint32_t)sink.n;
  *stripe_bits_out = sink.n + data_bits + 3;
  return TT_OK;
}

}  // namespace

extern "C" int64_t tt_png_stream_bytes(int32_t h, int32_t w, int32_t ch) {
  return tt_png_shape_ok(1, h, w, ch) ? (int64_t)h * (1 + (int64_t)w * ch) : 0;
}
extern "C" int64_t tt_png_frame_stride(int32_t h, int32_t w, int32_t ch) { return (tt_png_stream_bytes(h, w, ch) + 15) / 16 * 16; }
extern "C" int64_t tt_png_stripes(int32_t h, int32_t w, int32_t ch) { return (tt_png_stream_bytes(h, w, ch) + TT_PNG_STRIPE - 1) / TT_PNG_STRIPE; }

extern "C" int tt_png_code_lengths(const uint32_t* counts, int32_t nsym, int32_t limit, uint8_t* lengths) {
  if (!counts || !lengths) TT_FAIL(TT_EINVAL, "tt_png_code_lengths: null %s", !counts ? "counts" : "lengths");
  if (nsym < 1 || nsym > TT_PNG_SYMS) TT_FAIL(TT_EINVAL, "tt_png_code_lengths: nsym = %d (1 to %d)", nsym, TT_PNG_SYMS);
  if (limit < 1 || limit > TT_PNG_LIT_LIMIT) TT_FAIL(TT_EINVAL, "tt_png_code_lengths: limit = %d (1 to %d)", limit, TT_PNG_LIT_LIMIT);
  return tt_code_lengths("tt_png_code_lengths", counts, nsym, limit, lengths);
}

extern "C" int tt_png_block_header(const uint32_t* counts, const uint8_t* lengths, uint32_t* header, int32_t cap_words, int64_t* stripe_bits_out) {
  if (!counts || !lengths || !header || !stripe_bits_out)
    TT_FAIL(TT_EINVAL, "tt_png_block_header: null %s", !counts ? "counts" : (!lengths ? "lengths" : (!header ? "header" : "stripe_bits_out")));
  return block_header("tt_png_block_header", counts, lengths, header, cap_words, stripe_bits_out);
}

extern "C" int tt_png_plan(const uint32_t* records, int64_t nstripes, uint32_t* tables, uint32_t* headers, int64_t* total_bytes_out) {
  if (!records || !tables || !headers || !total_bytes_out)
    TT_FAIL(TT_EINVAL, "tt_png_plan: null %s", !records ? "records" : (!tables ? "tables" : (!headers ? "headers" : "total_bytes_out")));
  if (nstripes <= 0) TT_FAIL(TT_EINVAL, "tt_png_plan: nstripes = %lld", (long long)nstripes);
  int64_t offset = 0;
  uint8_t lengths[TT_PNG_SYMS];
  for (int64_t i = 0; i < nstripes; ++i) {
    const uint32_t* counts = records + i * TT_PNG_RECORD_WORDS;
    uint32_t* table = tables + i * TT_PNG_TABLE_WORDS;
    uint64_t tokens = 0;
    for (int s = 0; s < TT_PNG_SYMS; ++s) tokens += counts[s];
    if (counts[256] != 1 || tokens < 2 || tokens > TT_PNG_STRIPE + 1)
      TT_FAIL(TT_EINVAL, "tt_png_plan: record %lld is not a stripe's (end-of-block count %u, %llu tokens)", (long long)i, counts[256], (unsigned long long)tokens);
    int rc = tt_code_lengths("tt_png_plan", counts, TT_PNG_SYMS, TT_PNG_LIT_LIMIT, lengths);
    if (rc != TT_OK) return rc;
    int64_t bits = 0;
    rc = block_header("tt_png_plan", counts, lengths, headers + i * TT_PNG_HEADER_WORDS, TT_PNG_HEADER_WORDS, &bits);
    if (rc != TT_OK) return rc;
    reversed_codes(lengths, TT_PNG_SYMS, table);
    for (int s = 0; s < TT_PNG_SYMS; ++s) table[s] |= (uint32_t)lengths[s] << 16;
    table[286] = (uint32_t)((uint64_t)offset & 0xffffffffu);
    table[287] = (uint32_t)((uint64_t)offset >> 32);
    offset += (bits + 7) / 8 + 4;
  }
  *total_bytes_out = offset;
  return TT_OK;
}

// ---- the PNG import's host half (include/ttvdm.h, "PNG import", rule 1): the container walked chunk by chunk
namespace {

uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3]; }

uint32_t crc32_of(const uint8_t* p, int64_t n) {                 // the CRC-32 of PNG (ISO 3309), bit by bit: IHDR's 17 bytes only
  uint32_t c = 0xffffffffu;
  for (int64_t i = 0; i < n; ++i) {
    c ^= p[i];
    for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1u)));
  }
  return c ^ 0xffffffffu;
}

struct ZlibHead {                                  // the first two bytes of a zlib stream, gathered across chunk boundaries
  int have;
  uint8_t b[2];
  void feed(const uint8_t* p, int64_t n) {
    for (int64_t i = 0; i < n && have < 2; ++i) b[have++] = p[i];
  }
};

int zlib_head_ok(const char* who, const ZlibHead& z, const char* what, int frame) {
  char where[48];
  if (frame < 0) snprintf(where, sizeof where, "%s", what);
  else snprintf(where, sizeof where, "frame %d", frame);
  if (z.have < 2) TT_FAIL(TT_EINVAL, "%s: %s holds no zlib header (a stream of fewer than 2 bytes; method 8 is what PNG allows)", who, where);
  if ((z.b[0] & 15) != 8) TT_FAIL(TT_EINVAL, "%s: %s: a zlib header of method %d, not method 8 (deflate)", who, where, z.b[0] & 15);
  if ((z.b[0] >> 4) > 7) TT_FAIL(TT_EINVAL, "%s: %s: a zlib header that names a window of 2^%d bytes (32 KiB at the most)", who, where, (z.b[0] >> 4) + 8);
  if (z.b[1] & 0x20) TT_FAIL(TT_EINVAL, "%s: %s: a zlib header with a preset dictionary", who, where);
  if ((((int)z.b[0] << 8) + z.b[1]) % 31) TT_FAIL(TT_EINVAL, "%s: %s: a zlib header that fails its check bits", who, where);
  return TT_OK;
}

}  // namespace

extern "C" int tt_png_parse(const uint8_t* data, int64_t size, TtPngHeader* header, TtPngSpan* spans, int64_t span_cap, TtPngFrame* frames,
                            int64_t frame_cap, uint8_t* upload, int64_t upload_cap) {
  const char* who = "tt_png_parse";
  static const uint8_t SIG[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
  if (!data) TT_FAIL(TT_EINVAL, "%s: null data", who);
  if (!header) TT_FAIL(TT_EINVAL, "%s: null header", who);
  if (size <= 0) TT_FAIL(TT_EINVAL, "%s: size = %lld", who, (long long)size);
  const bool fill = spans || frames || upload;
  if (fill && (!spans || !upload)) TT_FAIL(TT_EINVAL, "%s: spans, frames and upload go together (all NULL counts)", who);
  if (size < 8 || memcmp(data, SIG, 8) != 0) TT_FAIL(TT_EINVAL, "%s: not a PNG file (a bad signature)", who);
  TtPngHeader hd;
  memset(&hd, 0, sizeof hd);
  hd.plays = -1;
  hd.idat_offset = -1;
  bool ended = false, idat_open = false, idat_closed = false;
  int64_t nspans = 0, nframes = 0, at = 0;          // at: bytes copied so far
  ZlibHead idat_head = {0, {0, 0}}, frame_head = {0, {0, 0}};
  int64_t pos = 8;
  for (int64_t chunk = 0; pos < size && !ended; ++chunk) {        // every trip passes 12 bytes or more
    if (size - pos < 12) TT_FAIL(TT_EINVAL, "%s: the file ends inside a chunk's frame at byte %lld", who, (long long)pos);
    const uint32_t len = be32(data + pos);
    const uint8_t* type = data + pos + 4;
    if (len > 0x7fffffffu || (int64_t)len > size - pos - 12)
      TT_FAIL(TT_EINVAL, "%s: the file ends inside the %.4s chunk at byte %lld (%u bytes announced)", who, (const char*)type, (long long)pos, len);
    const uint8_t* body = data + pos + 8;
    auto named = [&](const char* t) { return memcmp(type, t, 4) == 0; };
    if (chunk == 0) {
      if (!named("IHDR")) TT_FAIL(TT_EINVAL, "%s: the first chunk is %.4s, not IHDR (a missing IHDR)", who, (const char*)type);
      if (len != 13) TT_FAIL(TT_EINVAL, "%s: an IHDR of %u bytes, not 13", who, len);
      if (crc32_of(type, 17) != be32(body + 13)) TT_FAIL(TT_EINVAL, "%s: IHDR's CRC does not match", who);
      const uint32_t w = be32(body), h = be32(body + 4);
      const int depth = body[8], color = body[9];
      if (w == 0 || h == 0 || w > 0x7fffffffu || h > 0x7fffffffu) TT_FAIL(TT_EINVAL, "%s: an image of zero size (%u x %u)", who, w, h);
      if (color == 3) TT_FAIL(TT_EUNSUPPORTED, "%s: a palette file (colour type 3)", who);
      if (color != 0 && color != 2 && color != 4 && color != 6) TT_FAIL(TT_EINVAL, "%s: colour type %d is none of PNG's", who, color);
      if (depth != 8) TT_FAIL(TT_EUNSUPPORTED, "%s: bit depth %d (8 is what is decoded)", who, depth);
      if (body[10] != 0 || body[11] != 0) TT_FAIL(TT_EUNSUPPORTED, "%s: compression method %d, filter method %d (0 and 0 are PNG's)", who, body[10], body[11]);
      if (body[12] != 0) TT_FAIL(TT_EUNSUPPORTED, "%s: an interlaced (Adam7) file", who);
      hd.width = (int32_t)w;
      hd.height = (int32_t)h;
      hd.bit_depth = depth;
      hd.color_type = color;
      hd.channels = color == 0 ? 1 : (color == 4 ? 2 : (color == 2 ? 3 : 4));
    } else if (named("IDAT")) {
      if (idat_closed) TT_FAIL(TT_EINVAL, "%s: IDAT chunks apart (another chunk stands between them)", who);
      if (!idat_open) {
        idat_open = true;
        hd.idat_offset = at;
        if (nframes > 0) {                                         // an fcTL before the IDAT: the default image is frame 0
          hd.default_is_frame = 1;
          if (fill) frames[0].data_offset = at;
        }
      }
      if (fill) {
        if (nspans >= span_cap) TT_FAIL(TT_EINVAL, "%s: span_cap too small (%lld)", who, (long long)span_cap);
        if ((int64_t)len > upload_cap - at) TT_FAIL(TT_EINVAL, "%s: upload_cap too small (%lld)", who, (long long)upload_cap);
        const TtPngSpan sp = {pos + 8, (int64_t)len, hd.default_is_frame ? 0 : -1, 0};
        spans[nspans] = sp;
        if (len) memcpy(upload + at, body, len);
        if (hd.default_is_frame) { frames[0].data_bytes += len; ++frames[0].spans; }
      }
      idat_head.feed(body, len);
      ++nspans;
      at += len;
      hd.idat_bytes += len;
    } else {
      if (idat_open) idat_closed = true;
      if (named("IEND")) ended = true;
      else if (named("acTL")) {
        if (len != 8) TT_FAIL(TT_EINVAL, "%s: an acTL of %u bytes, not 8", who, len);
        hd.announced = (int32_t)(be32(body) & 0x7fffffffu);
        hd.plays = (int32_t)(be32(body + 4) & 0x7fffffffu);
      } else if (named("fcTL")) {
        if (len != 26) TT_FAIL(TT_EINVAL, "%s: an fcTL of %u bytes, not 26", who, len);
        if (!idat_open && nframes > 0) TT_FAIL(TT_EINVAL, "%s: two fcTL chunks before the IDAT", who);
        if (nframes > 0 && !(nframes == 1 && hd.default_is_frame)) {                      // the frame before is complete: its stream's header
          const int rc = zlib_head_ok(who, frame_head, "IDAT", (int)(nframes - 1));
          if (rc != TT_OK) return rc;
        }
        if (nframes >= 65535) TT_FAIL(TT_EUNSUPPORTED, "%s: more than 65535 frames", who);
        frame_head.have = 0;
        if (fill) {
          if (!frames || nframes >= frame_cap) TT_FAIL(TT_EINVAL, "%s: frame_cap too small (%lld)", who, (long long)frame_cap);
          TtPngFrame fr;
          memset(&fr, 0, sizeof fr);
          fr.sequence = (int32_t)(be32(body) & 0x7fffffffu);
          fr.width = (int32_t)(be32(body + 4) & 0x7fffffffu);
          fr.height = (int32_t)(be32(body + 8) & 0x7fffffffu);
          fr.x = (int32_t)(be32(body + 12) & 0x7fffffffu);
          fr.y = (int32_t)(be32(body + 16) & 0x7fffffffu);
          fr.delay_num = (body[20] << 8) | body[21];
          fr.delay_den = (body[22] << 8) | body[23];
          fr.dispose = body[24];
          fr.blend = body[25];
          fr.data_offset = at;
          frames[nframes] = fr;
        }
        ++nframes;
      } else if (named("fdAT")) {
        if (nframes == 0 || !idat_open) TT_FAIL(TT_EINVAL, "%s: an fdAT chunk before any fcTL or before the IDAT", who);
        if (len < 4) TT_FAIL(TT_EINVAL, "%s: an fdAT of %u bytes (4 at the least: its sequence number)", who, len);
        if (fill) {
          if (nspans >= span_cap) TT_FAIL(TT_EINVAL, "%s: span_cap too small (%lld)", who, (long long)span_cap);
          if ((int64_t)len - 4 > upload_cap - at) TT_FAIL(TT_EINVAL, "%s: upload_cap too small (%lld)", who, (long long)upload_cap);
          const TtPngSpan sp = {pos + 12, (int64_t)len - 4, (int32_t)(nframes - 1), 0};
          spans[nspans] = sp;
          if (len > 4) memcpy(upload + at, body + 4, len - 4);
          frames[nframes - 1].data_bytes += len - 4;
          ++frames[nframes - 1].spans;
        }
        frame_head.feed(body + 4, (int64_t)len - 4);
        ++nspans;
        at += len - 4;
      } else if (!(type[0] & 0x20) && !named("PLTE")) {
        TT_FAIL(TT_EINVAL, "%s: an unknown critical chunk %.4s at byte %lld", who, (const char*)type, (long long)pos);
      }
    }
    pos += 12 + (int64_t)len;
  }
  if (!ended) TT_FAIL(TT_EINVAL, "%s: the file ends inside its chunks: no IEND after %lld bytes", who, (long long)size);
  if (!idat_open) TT_FAIL(TT_EINVAL, "%s: no IDAT chunk", who);
  if (hd.idat_bytes >= (1ll << 29) || at >= (1ll << 29)) TT_FAIL(TT_EUNSUPPORTED, "%s: %lld bytes of compressed data (fewer than 2^29)", who, (long long)at);
  int rc = zlib_head_ok(who, idat_head, "IDAT", -1);
  if (rc != TT_OK) return rc;
  if (nframes > 0 && !(nframes == 1 && hd.default_is_frame)) {
    rc = zlib_head_ok(who, frame_head, "IDAT", (int)(nframes - 1));
    if (rc != TT_OK) return rc;
  }
  hd.spans = (int32_t)nspans;
  hd.frames = (int32_t)nframes;
  hd.data_bytes = at;
  *header = hd;
  return TT_OK;
}
