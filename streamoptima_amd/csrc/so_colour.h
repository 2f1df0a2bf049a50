// so_colour.h — argument block and integer tables of the colour conversion kernels
// (so_colour.hip; the arithmetic is stated in include/streamoptima.h, "Colour conversion").
#pragma once
#include "so_common.h"

namespace so {

constexpr int kColourBatch = 32;     // frames per launch (device pointers by value)
constexpr int kColourThreads = 256;
constexpr int kColourCellW = 8;      // a lane's cell: 2 rows of 8 pixels, 4 chroma samples of U and of V

// Table index: SO_COLOUR_BT601 / SO_COLOUR_BT709 times 2, plus 1 for limited range.
// Forward, rows Y, Cb, Cr and columns R, G, B, 16 fractional bits: rint(coef * 65536) with the G
// entry carrying what makes the Y row sum to rint(ys * 65536) and the chroma rows to 0.
constexpr int32_t kColourFwd[4][9] = {
    {19595, 38470, 7471, -11058, -21710, 32768, 32768, -27439, -5329},   // 601 full
    {16829, 33039, 6416, -9714, -19070, 28784, 28784, -24103, -4681},    // 601 limited
    {13933, 46871, 4732, -7509, -25259, 32768, 32768, -29763, -3005},    // 709 full
    {11966, 40254, 4064, -6596, -22188, 28784, 28784, -26145, -2639},    // 709 limited
};
// Inverse, rows R, G, B and columns Y - yoff, U - 128, V - 128: rint(M * 65536), unadjusted.
constexpr int32_t kColourInv[4][9] = {
    {65536, 0, 91881, 65536, -22553, -46802, 65536, 116130, 0},          // 601 full
    {76309, 0, 104597, 76309, -25675, -53279, 76309, 132201, 0},         // 601 limited
    {65536, 0, 103206, 65536, -12276, -30679, 65536, 121609, 0},         // 709 full
    {76309, 0, 117489, 76309, -13975, -34925, 76309, 138438, 0},         // 709 limited
};

struct ColourPtrs {
    uint8_t* rgb[kColourBatch];   // read by the forward kernel, written by the inverse one
    uint8_t* y[kColourBatch];     // the other way round
    uint8_t* u[kColourBatch];
    uint8_t* v[kColourBatch];
};

struct ColourGeom {
    int32_t h, w;            // picture
    int32_t Hp, Wp;          // padded luma plane (pitch Wp; chroma planes Hp/2 x Wp/2, pitch Wp/2)
    size_t pitch, plane;     // RGB: bytes from row to row; chw: bytes from plane to plane
    int32_t c[9];            // the table row in use
    int32_t yoff;            // 0 or 16
};

int colour_forward_launch(int layout, const uint8_t* const* rgb, uint8_t* const* y, uint8_t* const* u,
                          uint8_t* const* v, int nframes, const ColourGeom& g, hipStream_t st);
int colour_inverse_launch(int layout, const uint8_t* const* y, const uint8_t* const* u, const uint8_t* const* v,
                          uint8_t* const* rgb, int nframes, const ColourGeom& g, hipStream_t st);

}  // namespace so
