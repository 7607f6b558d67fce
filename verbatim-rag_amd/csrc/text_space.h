// Python's Unicode white space (str.isspace, the `\s` of `re` on str) over UTF-8 bytes, shared by the byte-level text kernels
// (text.hip: sentence split; chunk.hip: markdown headers): U+0009-000D, U+001C-0020, U+0085, U+00A0, U+1680, U+2000-200A,
// U+2028, U+2029, U+202F, U+205F, U+3000.
#pragma once
#include <hip/hip_runtime.h>

namespace vrag {

// Length in bytes of the white-space character that starts at p[0] (n bytes are readable), 0 if it is not white space.
__device__ __forceinline__ int space_len(const unsigned char* p, long long n) {
  const unsigned c = p[0];
  if ((c >= 0x09 && c <= 0x0D) || (c >= 0x1C && c <= 0x20)) return 1;
  if (c == 0xC2 && n >= 2) return (p[1] == 0x85 || p[1] == 0xA0) ? 2 : 0;
  if (n < 3) return 0;
  if (c == 0xE1) return (p[1] == 0x9A && p[2] == 0x80) ? 3 : 0;                                         // U+1680
  if (c == 0xE2) {
    if (p[1] == 0x80) return (p[2] <= 0x8A && p[2] >= 0x80) || p[2] == 0xA8 || p[2] == 0xA9 || p[2] == 0xAF ? 3 : 0;   // U+2000-200A, 2028, 2029, 202F
    if (p[1] == 0x81) return p[2] == 0x9F ? 3 : 0;                                                     // U+205F
    return 0;
  }
  if (c == 0xE3) return (p[1] == 0x80 && p[2] == 0x80) ? 3 : 0;                                         // U+3000
  return 0;
}

}  // namespace vrag
