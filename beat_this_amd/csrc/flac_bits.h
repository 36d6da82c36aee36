// FLAC bit reader, frame-header parser and subframe walker (include/beat_this_amd.h, "FLAC decode"): ONE text for the host
// twin and the kernels of csrc/flac.hip.  Everything here is __host__ __device__ inline code over a track's bytes [0, n):
// every read is checked against that range, and a read past the end yields "invalid", never a load.
//
// The walker is written once and instantiated twice: with a sink that is not ACTIVE it only measures a frame (where it
// ends, whether its padding and CRC-16 hold), with an ACTIVE sink it restores the samples.  A sink supplies the storage the
// predictor recurrence needs -- the LPC coefficients and a ring of the last 32 restored samples -- so that neither is a
// runtime-indexed register array on the device (those go to scratch): the kernels keep both in LDS, the host twin on its stack.
#pragma once

#include <cstdint>

#ifndef __HIPCC__
#define __host__
#define __device__
#define __forceinline__ inline
#endif

#define FL_HD __host__ __device__ __forceinline__

namespace flac {

// what the metadata says about a stream (bt_flac_info: the same layout, asserted in flac.hip)
struct Info {
  int32_t sample_rate, channels, bps, blocking;   // blocking: the first frame's blocking bit
  int32_t min_block, max_block;
  int64_t total_samples, first_frame, n_bytes;
  uint8_t md5[16];
};

struct Header {
  int32_t block;       // samples per channel in this frame
  int32_t assign;      // channel assignment 0 .. 10
  int32_t bytes;       // length of the header, CRC-8 included
  uint64_t number;     // frame number (fixed blocking) or first sample (variable)
};

// ---- bits -----------------------------------------------------------------------------------------------------------------
// A 64-bit window, most significant bit first, refilled bytewise from any alignment.  Invariant: the bits of ``win`` below
// the top ``cnt`` are zero.
struct Bits {
  const uint8_t* s;
  int64_t n, byte;     // ``byte``: the next byte to put into the window
  uint64_t win;
  int cnt;
  bool bad;

  FL_HD void open(const uint8_t* src, int64_t n_bytes, int64_t at) {
    s = src, n = n_bytes, byte = at, win = 0, cnt = 0, bad = at < 0 || at > n_bytes;
    if (bad) byte = n;
  }
  FL_HD void refill() {
    while (cnt <= 56 && byte < n) {
      win |= (uint64_t)s[byte++] << (56 - cnt);
      cnt += 8;
    }
  }
  // k in 0 .. 32
  FL_HD uint32_t read(int k) {
    if (k == 0) return 0;
    refill();
    if (cnt < k) {
      bad = true;
      return 0;
    }
    const uint32_t v = (uint32_t)(win >> (64 - k));
    win <<= k;
    cnt -= k;
    return v;
  }
  FL_HD int32_t read_signed(int k) {
    if (k == 0) return 0;
    const uint32_t v = read(k);
    return (int32_t)(v << (32 - k)) >> (32 - k);
  }
  // zeros up to the next 1, which is consumed too: a run may be far longer than the window
  FL_HD uint32_t unary() {
    uint32_t q = 0;
    for (;;) {
      refill();
      if (cnt == 0) {
        bad = true;
        return 0;
      }
      if (win == 0) {
        q += (uint32_t)cnt;
        cnt = 0;
        continue;
      }
#ifdef __HIP_DEVICE_COMPILE__
      const int lz = __clzll((long long)win);
#else
      const int lz = __builtin_clzll(win);
#endif
      q += (uint32_t)lz;
      win = lz == 63 ? 0 : win << (lz + 1);
      cnt -= lz + 1;
      return q;
    }
  }
  FL_HD bool aligned() const { return (cnt & 7) == 0; }
  FL_HD int64_t byte_pos() const { return byte - (cnt >> 3); }   // (of an aligned reader)
};

FL_HD uint32_t crc8(const uint8_t* p, int len) {
  uint32_t c = 0;
  for (int i = 0; i < len; ++i) {
    c ^= p[i];
    for (int b = 0; b < 8; ++b) c = (c & 0x80) ? ((c << 1) ^ 0x07) & 0xFF : (c << 1) & 0xFF;
  }
  return c;
}

FL_HD uint32_t crc16(const uint8_t* p, int64_t len) {
  uint32_t c = 0;
  for (int64_t i = 0; i < len; ++i) {
    c ^= (uint32_t)p[i] << 8;
    for (int b = 0; b < 8; ++b) c = (c & 0x8000) ? ((c << 1) ^ 0x8005) & 0xFFFF : (c << 1) & 0xFFFF;
  }
  return c;
}

// ---- the frame header -------------------------------------------------------------------------------------------------------
// A frame header of THIS stream at byte ``at``: the sync, the stream's blocking bit, no reserved code, channel count, sample
// size and rate as STREAMINFO has them, a block size up to max_block, a well-formed coded number, CRC-8.
FL_HD bool parse_header(const uint8_t* s, int64_t n, int64_t at, const Info& in, Header& h) {
  if (at < 0 || at + 5 > n) return false;   // (the shortest header is 5 bytes before its CRC-8)
  const uint8_t* p = s + at;
  if (p[0] != 0xFF || p[1] != (0xF8 | (in.blocking & 1))) return false;
  const int bs_code = p[2] >> 4, sr_code = p[2] & 15, assign = p[3] >> 4, ss_code = (p[3] >> 1) & 7;
  if ((p[3] & 1) || bs_code == 0 || sr_code == 15 || assign > 10 || ss_code == 3 || ss_code == 7) return false;
  if ((assign < 8 ? assign + 1 : 2) != in.channels) return false;
  if (ss_code) {
    const int bits = ss_code == 1 ? 8 : ss_code == 2 ? 12 : ss_code == 4 ? 16 : ss_code == 5 ? 20 : 24;
    if (bits != in.bps) return false;
  }
  // the coded number: UTF-8's scheme, up to 7 bytes
  const uint32_t b0 = p[4];
  int extra;
  uint64_t num;
  if (b0 < 0x80) extra = 0, num = b0;
  else if (b0 < 0xC0) return false;
  else if (b0 < 0xE0) extra = 1, num = b0 & 0x1F;
  else if (b0 < 0xF0) extra = 2, num = b0 & 0x0F;
  else if (b0 < 0xF8) extra = 3, num = b0 & 0x07;
  else if (b0 < 0xFC) extra = 4, num = b0 & 0x03;
  else if (b0 < 0xFE) extra = 5, num = b0 & 0x01;
  else if (b0 == 0xFE) extra = 6, num = 0;
  else return false;
  int len = 5 + extra + (bs_code == 6 ? 1 : bs_code == 7 ? 2 : 0) + (sr_code == 12 ? 1 : sr_code >= 13 ? 2 : 0);
  if (at + len + 1 > n) return false;
  for (int i = 0; i < extra; ++i) {
    const uint32_t b = p[5 + i];
    if ((b & 0xC0) != 0x80) return false;
    num = (num << 6) | (b & 0x3F);
  }
  int q = 5 + extra;
  int block;
  if (bs_code == 1) block = 192;
  else if (bs_code <= 5) block = 576 << (bs_code - 2);
  else if (bs_code == 6) block = p[q] + 1, q += 1;
  else if (bs_code == 7) block = ((p[q] << 8) | p[q + 1]) + 1, q += 2;
  else block = 256 << (bs_code - 8);
  if (block > in.max_block || block > 65535) return false;
  int rate;
  switch (sr_code) {
    case 0: rate = in.sample_rate; break;
    case 1: rate = 88200; break;
    case 2: rate = 176400; break;
    case 3: rate = 192000; break;
    case 4: rate = 8000; break;
    case 5: rate = 16000; break;
    case 6: rate = 22050; break;
    case 7: rate = 24000; break;
    case 8: rate = 32000; break;
    case 9: rate = 44100; break;
    case 10: rate = 48000; break;
    case 11: rate = 96000; break;
    case 12: rate = p[q] * 1000, q += 1; break;
    case 13: rate = (p[q] << 8) | p[q + 1], q += 2; break;
    default: rate = ((p[q] << 8) | p[q + 1]) * 10, q += 2; break;
  }
  if (rate != in.sample_rate) return false;
  if (crc8(p, len) != p[len]) return false;
  h.block = block, h.assign = assign, h.bytes = len + 1, h.number = num;
  return true;
}

// ---- sinks ------------------------------------------------------------------------------------------------------------------
// What the walker needs from a sink S:
//   S::ACTIVE                          false: measure only, nothing below is called
//   set_coef(j, v), coef(j)            the LPC coefficients, j in 0 .. 31
//   put(c, i, v, wasted), hist(i)      sample i of channel c restored as v (before the wasted bits' shift); hist(i) returns
//                                      one of the last 32 samples put for the current channel
struct NullSink {
  static constexpr bool ACTIVE = false;
  FL_HD void set_coef(int, int32_t) {}
  FL_HD int32_t coef(int) const { return 0; }
  FL_HD void put(int, int, int32_t, int) {}
  FL_HD int32_t hist(int) const { return 0; }
};

// Samples go to a planar int32 array (channel c of the frame at pl + c ld) at their true positions, the stereo decorrelation
// undone as the second channel arrives (the first one was written by this same walker).  ``Store`` holds the coefficients and
// the ring: Store::cf(j), Store::ring(i) -> int32_t&.
template <class Store> struct PlanarSink {
  static constexpr bool ACTIVE = true;
  Store st;
  int32_t* pl;
  int64_t ld;
  int assign;
  FL_HD void set_coef(int j, int32_t v) { st.cf(j) = v; }
  FL_HD int32_t coef(int j) { return st.cf(j); }
  FL_HD int32_t hist(int i) { return st.ring(i & 31); }
  FL_HD void put(int c, int i, int32_t v, int wasted) {
    st.ring(i & 31) = v;
    const int32_t x = (int32_t)((uint32_t)v << wasted);
    if (assign < 8 || c == 0) {
      pl[c * ld + i] = x;
    } else if (assign == 8) {          // left, side  (unsigned: a forged frame wraps, it does not overflow)
      pl[ld + i] = (int32_t)((uint32_t)pl[i] - (uint32_t)x);
    } else if (assign == 9) {          // side, right
      pl[i] = (int32_t)((uint32_t)pl[i] + (uint32_t)x);
      pl[ld + i] = x;
    } else {                           // mid, side
      const uint32_t m = ((uint32_t)pl[i] << 1) | ((uint32_t)x & 1);
      pl[i] = (int32_t)(m + (uint32_t)x) >> 1;
      pl[ld + i] = (int32_t)(m - (uint32_t)x) >> 1;
    }
  }
};

// ---- subframes ----------------------------------------------------------------------------------------------------------------
FL_HD int ceil_log2(int v) {
  int r = 0;
  while ((1 << r) < v) ++r;
  return r;
}

// one restored sample from its residual: kind 0 = fixed, 1 = LPC
template <class S> FL_HD int32_t predict(S& sink, int kind, int order, int shift, bool wide, int i) {
  if (kind == 0) {
    switch (order) {
      case 0: return 0;
      case 1: return sink.hist(i - 1);
      case 2: return (int32_t)(2u * (uint32_t)sink.hist(i - 1) - (uint32_t)sink.hist(i - 2));
      case 3: return (int32_t)(3u * (uint32_t)sink.hist(i - 1) - 3u * (uint32_t)sink.hist(i - 2) + (uint32_t)sink.hist(i - 3));
      default:
        return (int32_t)(4u * (uint32_t)sink.hist(i - 1) - 6u * (uint32_t)sink.hist(i - 2) + 4u * (uint32_t)sink.hist(i - 3) -
                         (uint32_t)sink.hist(i - 4));
    }
  }
  if (wide) {   // bps + precision + log2(order) can pass 32 bits
    uint64_t acc = 0;
    for (int j = 0; j < order; ++j) acc += (uint64_t)((int64_t)sink.coef(j) * (int64_t)sink.hist(i - 1 - j));
    return (int32_t)((int64_t)acc >> shift);
  }
  uint32_t acc = 0;
  for (int j = 0; j < order; ++j) acc += (uint32_t)sink.coef(j) * (uint32_t)sink.hist(i - 1 - j);
  return (int32_t)acc >> shift;
}

// the residual of samples [order, block) of a subframe; every residual becomes a sample at once (ACTIVE) or is only skipped
template <class S> FL_HD bool walk_residual(Bits& b, S& sink, int c, int block, int kind, int order, int shift, bool wide, int wasted) {
  const uint32_t method = b.read(2);
  const int p = (int)b.read(4);
  if (b.bad || method > 1) return false;
  const int pbits = method ? 5 : 4, esc = method ? 31 : 15;
  if ((block & ((1 << p) - 1)) || (block >> p) < order) return false;
  int i = order;
  for (int part = 0; part < (1 << p); ++part) {
    const int cnt = (block >> p) - (part ? 0 : order);
    const int k = (int)b.read(pbits);
    if (b.bad) return false;
    if (k == esc) {
      const int w = (int)b.read(5);
      for (int t = 0; t < cnt; ++t, ++i) {
        const int32_t r = b.read_signed(w);
        if (b.bad) return false;
        if (S::ACTIVE) sink.put(c, i, (int32_t)((uint32_t)predict(sink, kind, order, shift, wide, i) + (uint32_t)r), wasted);
      }
    } else {
      for (int t = 0; t < cnt; ++t, ++i) {
        const uint32_t q = b.unary();
        const uint32_t low = b.read(k);
        if (b.bad) return false;
        if (S::ACTIVE) {
          const uint64_t u = ((uint64_t)q << k) | low;
          const uint32_t r = (u & 1) ? ~(uint32_t)(u >> 1) : (uint32_t)(u >> 1);   // -(u >> 1) - 1 for odd u
          sink.put(c, i, (int32_t)((uint32_t)predict(sink, kind, order, shift, wide, i) + r), wasted);
        }
      }
    }
  }
  return !b.bad;
}

// one subframe of ``block`` samples; ``bps`` = the frame's sample size, plus 1 for a side channel
template <class S> FL_HD bool walk_subframe(Bits& b, S& sink, int c, int block, int bps) {
  const uint32_t head = b.read(8);
  if (b.bad || (head & 0x80)) return false;
  const int type = (head >> 1) & 0x3F;
  int wasted = 0;
  if (head & 1) {
    const uint32_t k = b.unary();
    if (b.bad || k >= 32) return false;
    wasted = (int)k + 1;
  }
  const int width = bps - wasted;
  if (width < 1) return false;
  if (type == 0) {                                        // constant
    const int32_t v = b.read_signed(width);
    if (S::ACTIVE)
      for (int i = 0; i < block; ++i) sink.put(c, i, v, wasted);
    return !b.bad;
  }
  if (type == 1) {                                        // verbatim
    for (int i = 0; i < block; ++i) {
      const int32_t v = b.read_signed(width);
      if (b.bad) return false;
      if (S::ACTIVE) sink.put(c, i, v, wasted);
    }
    return true;
  }
  int kind, order;
  if (type >= 8 && type <= 12) kind = 0, order = type - 8;
  else if (type >= 32) kind = 1, order = type - 31;
  else return false;                                      // reserved
  if (order > block) return false;
  for (int i = 0; i < order; ++i) {
    const int32_t v = b.read_signed(width);
    if (b.bad) return false;
    if (S::ACTIVE) sink.put(c, i, v, wasted);
  }
  int shift = 0;
  bool wide = false;
  if (kind == 1) {
    const int prec = (int)b.read(4) + 1;
    shift = b.read_signed(5);
    if (b.bad || prec == 16 || shift < 0) return false;
    for (int j = 0; j < order; ++j) {
      const int32_t v = b.read_signed(prec);
      if (S::ACTIVE) sink.set_coef(j, v);
    }
    if (b.bad) return false;
    wide = width + prec + ceil_log2(order) > 32;
  }
  return walk_residual(b, sink, c, block, kind, order, shift, wide, wasted);
}

// The frame whose (already parsed) header ``h`` starts at byte ``at``: all subframes, the zero padding and the CRC-16.
// -> the byte behind the frame, or 0 where the frame is not valid.  An ACTIVE sink has then received every sample.
// ``check_crc`` false: a frame that was measured before is walked again.
template <class S> FL_HD int64_t walk_frame(const uint8_t* s, int64_t n, int64_t at, const Info& in, const Header& h, S& sink, bool check_crc) {
  Bits b;
  b.open(s, n, at + h.bytes);
  const int nch = h.assign < 8 ? h.assign + 1 : 2;
  for (int c = 0; c < nch; ++c) {
    const bool side = (h.assign == 8 && c == 1) || (h.assign == 9 && c == 0) || (h.assign == 10 && c == 1);
    if (!walk_subframe(b, sink, c, h.block, in.bps + (side ? 1 : 0))) return 0;
  }
  if (b.cnt & 7) {
    if (b.read(b.cnt & 7) != 0 || b.bad) return 0;       // the padding is zero bits
  }
  const int64_t crc_at = b.byte_pos();
  const uint32_t want = b.read(16);
  if (b.bad) return 0;
  if (check_crc && crc16(s + at, crc_at - at) != want) return 0;
  return crc_at + 2;
}

// ---- the chain ----------------------------------------------------------------------------------------------------------------
#define FL_OK 0
#define FL_BROKEN 1       // no valid frame with the expected number at ``where``
#define FL_LENGTH 2       // the frame at ``where`` would pass total_samples
#define FL_CANDIDATES 3   // the device found more frame-header candidates than its workspace provides for

// the number the frame after (number, block) must carry
FL_HD uint64_t next_number(const Info& in, uint64_t number, int block) { return in.blocking ? number + (uint64_t)block : number + 1; }

// ---- the mix ------------------------------------------------------------------------------------------------------------------
// pcm.hip's channel mean on the planar integers: s = v / 2^(bps-1), exact in fp64
template <class Load> FL_HD float mix_value(Load v, int channels, double scale) {
  if (channels == 1) return (float)((double)v(0) * scale);
  double acc = 0.0 + (double)v(0) * scale;
  for (int c = 1; c < channels; ++c) acc = acc + (double)v(c) * scale;
  acc = acc / (double)channels;
  return (float)acc;
}

// ---- the host side: metadata and the sequential twin --------------------------------------------------------------------------
struct Status {
  int32_t code, n_frames;
  int64_t n_samples, where;
};

// marker, ID3v2 skip, metadata walk, STREAMINFO, the first frame's offset and blocking bit -> 1, or 0 for a file outside the subset
inline int probe(const uint8_t* s, int64_t n, Info* out) {
  if (!s || !out || n < 4) return 0;
  int64_t p = 0;
  if (n >= 10 && s[0] == 'I' && s[1] == 'D' && s[2] == '3') {
    if ((s[6] | s[7] | s[8] | s[9]) & 0x80) return 0;
    p = 10 + (((int64_t)s[6] << 21) | ((int64_t)s[7] << 14) | ((int64_t)s[8] << 7) | s[9]) + ((s[5] & 0x10) ? 10 : 0);
  }
  if (p + 4 > n || s[p] != 'f' || s[p + 1] != 'L' || s[p + 2] != 'a' || s[p + 3] != 'C') return 0;
  p += 4;
  Info in{};
  bool have = false;
  for (bool last = false; !last;) {
    if (p + 4 > n) return 0;
    last = s[p] & 0x80;
    const int type = s[p] & 0x7F;
    const int64_t len = ((int64_t)s[p + 1] << 16) | ((int64_t)s[p + 2] << 8) | s[p + 3];
    p += 4;
    if (p + len > n || type == 127) return 0;
    if (!have) {   // STREAMINFO comes first
      if (type != 0 || len != 34) return 0;
      const uint8_t* q = s + p;
      in.min_block = (q[0] << 8) | q[1];
      in.max_block = (q[2] << 8) | q[3];
      in.sample_rate = (q[10] << 12) | (q[11] << 4) | (q[12] >> 4);
      in.channels = ((q[12] >> 1) & 7) + 1;
      in.bps = (((q[12] & 1) << 4) | (q[13] >> 4)) + 1;
      in.total_samples = ((int64_t)(q[13] & 15) << 32) | ((int64_t)q[14] << 24) | ((int64_t)q[15] << 16) | ((int64_t)q[16] << 8) | q[17];
      for (int i = 0; i < 16; ++i) in.md5[i] = q[18 + i];
      have = true;
    } else if (type == 0) {
      return 0;
    }
    p += len;
  }
  if (in.total_samples <= 0 || in.bps < 4 || in.bps > 24 || in.sample_rate <= 0 || in.max_block < 1) return 0;
  if (p + 2 > n || s[p] != 0xFF || (s[p + 1] & 0xFE) != 0xF8) return 0;
  in.blocking = s[p + 1] & 1;
  in.first_frame = p;
  in.n_bytes = n;
  *out = in;
  return 1;
}

struct HostStore {
  int32_t c[32], r[32];
  FL_HD int32_t& cf(int j) { return c[j]; }
  FL_HD int32_t& ring(int i) { return r[i]; }
};

// frame after frame from first_frame on, into ``planar`` (channels rows of ld = total_samples rounded up to 4); nothing else is written
inline void decode_chain_host(const uint8_t* s, const Info& in, int32_t* planar, int64_t ld, Status* st) {
  int64_t p = in.first_frame, pos = 0;
  int32_t frames = 0;
  uint64_t expect = 0;
  int code = FL_OK;
  PlanarSink<HostStore> sink{};
  sink.ld = ld;
  while (pos < in.total_samples) {
    Header h;
    if (!parse_header(s, in.n_bytes, p, in, h) || (frames > 0 && h.number != expect)) {
      code = FL_BROKEN;
      break;
    }
    if (pos + h.block > in.total_samples) {
      code = FL_LENGTH;
      break;
    }
    sink.pl = planar + pos;
    sink.assign = h.assign;
    const int64_t end = walk_frame(s, in.n_bytes, p, in, h, sink, true);
    if (!end) {
      code = FL_BROKEN;
      break;
    }
    expect = next_number(in, h.number, h.block);
    pos += h.block;
    p = end;
    ++frames;
  }
  st->code = code, st->n_frames = frames, st->n_samples = pos, st->where = p;
}

}  // namespace flac
