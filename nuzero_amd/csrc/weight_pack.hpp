// Host-only pieces every weight packer shares (engine.hip pack_conv, boardnet.hip pack): the exact three-piece bf16
// split of a float32 weight, the 32-bit word two channels' pieces travel in, and the heads' channel schedule.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

namespace nz {

// a = p[0] + p[1] + p[2] exactly, each piece a bf16 number (the next 8 significant bits, truncated)
inline void split3(float a, uint16_t p[3]) {
  float r = a;
  for (int i = 0; i < 3; ++i) {
    uint32_t bits;
    memcpy(&bits, &r, 4);
    bits &= 0xFFFF0000u;
    p[i] = (uint16_t)(bits >> 16);
    float t;
    memcpy(&t, &bits, 4);
    r = r - t;
  }
}

// the pieces of two neighbouring input channels, one word per piece: the even channel's in the low half (a channel
// that is padding passes 0.f: all its pieces are zero bits)
inline void split3_pair(float even, float odd, uint32_t word[3]) {
  uint16_t lo[3], hi[3];
  split3(even, lo);
  split3(odd, hi);
  for (int piece = 0; piece < 3; ++piece) word[piece] = (uint32_t)lo[piece] | ((uint32_t)hi[piece] << 16);
}

// a float32 weight as ONE bf16, round to nearest even (the plain-bf16 mode's stream; the device rounds activations with
// v_cvt_pk_bf16_f32, the same rule).  Infinities and NaNs keep their upper half.
inline uint16_t bf16_rne(float a) {
  uint32_t bits;
  memcpy(&bits, &a, 4);
  if ((bits & 0x7F800000u) == 0x7F800000u) return (uint16_t)(bits >> 16) | ((bits & 0xFFFFu) ? 0x40u : 0u);
  return (uint16_t)((bits + 0x7FFFu + ((bits >> 16) & 1u)) >> 16);
}

// channels after each layer of a head that goes from `width` to `out` in `layers` steps (blocks.py:56-66,144-153)
inline std::vector<int> head_channels(int width, int out, int layers) {
  std::vector<int> ch{width};
  const double step = (double)(out - width) / layers;
  double prev = width;
  for (int i = 0; i < layers; ++i) { prev += step; ch.push_back((int)prev); }
  return ch;
}

}  // namespace nz
