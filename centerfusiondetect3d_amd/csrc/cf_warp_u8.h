// cv2.warpAffine(INTER_LINEAR, constant border 0) of one 8-bit pixel in OpenCV's fixed-point arithmetic (10-bit coordinates,
// 5-bit bilinear fractions, 15-bit weights: oracle/preprocess_ref.py states it).  Shared by the inference warp
// (cf_radar.hip: preprocess_kernel) and the training warp (cf_augment.hip), so that both round alike.
// Every file that includes this is built with -ffp-contract=off: M1*y + M2 must round twice, as it does in OpenCV.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// img (Hs, Ws, 3) uint8; m: the dst -> src map (already inverted); (x, y): the output pixel -> v[c], the 8-bit results.
// mirror: the source is read as img[:, ::-1, :] - coordinates, weights and the validity test are those of tap column j, only
// the column fetched is Ws-1-j (folding the mirror into the matrix would round the 5-bit fractions differently).
__device__ __forceinline__ void cf_warp_affine_u8(const uint8_t* __restrict__ img, int Hs, int Ws, const double (&m)[6], int x,
                                                  int y, bool mirror, int (&v)[3]) {
  const int X0 = __double2int_rn((m[1] * (double)y + m[2]) * 1024.0) + 16;
  const int Y0 = __double2int_rn((m[4] * (double)y + m[5]) * 1024.0) + 16;
  const int X = (X0 + __double2int_rn(m[0] * (double)x * 1024.0)) >> 5;
  const int Y = (Y0 + __double2int_rn(m[3] * (double)x * 1024.0)) >> 5;
  const int sx = X >> 5, sy = Y >> 5, fx = X & 31, fy = Y & 31;
  const int w00 = (32 - fx) * (32 - fy) * 32, w01 = fx * (32 - fy) * 32;
  const int w10 = (32 - fx) * fy * 32, w11 = fx * fy * 32;
  const bool y0 = (unsigned)sy < (unsigned)Hs, y1 = (unsigned)(sy + 1) < (unsigned)Hs;
  const bool x0 = (unsigned)sx < (unsigned)Ws, x1 = (unsigned)(sx + 1) < (unsigned)Ws;
  const int r0 = y0 ? sy : 0, r1 = y1 ? sy + 1 : 0;                   // (an invalid tap reads pixel 0 with weight 0)
  int c0 = x0 ? sx : 0, c1 = x1 ? sx + 1 : 0;
  if (mirror) {
    c0 = Ws - 1 - c0;
    c1 = Ws - 1 - c1;
  }
  const uint8_t* p00 = img + ((size_t)r0 * Ws + c0) * 3;
  const uint8_t* p01 = img + ((size_t)r0 * Ws + c1) * 3;
  const uint8_t* p10 = img + ((size_t)r1 * Ws + c0) * 3;
  const uint8_t* p11 = img + ((size_t)r1 * Ws + c1) * 3;
  const int m00 = (y0 && x0) ? w00 : 0, m01 = (y0 && x1) ? w01 : 0;
  const int m10 = (y1 && x0) ? w10 : 0, m11 = (y1 && x1) ? w11 : 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int acc = p00[c] * m00 + p01[c] * m01 + p10[c] * m10 + p11[c] * m11;
    v[c] = (acc + (1 << 14)) >> 15;
  }
}
