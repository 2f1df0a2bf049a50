// so_chroma.h — the argument block of the chroma kernels (so_chroma.hip), filled by the C-ABI
// entry points so_chroma_encode_frame / so_chroma_recon_frame (so_capi.hip).
#pragma once
#include "so_common.h"

namespace so {

struct ChromaPlanes {
    const uint8_t* cur;    // ENC only
    RefSet refs;           // P-frames only
    int16_t* qtc;          // ENC: written; !ENC: read
    uint8_t* recon;
};

struct ChromaArgs {
    ChromaPlanes pl[2];    // U, V
    int nref, Hc, Wc, nbx, nb, frame_type;
    const uint8_t* split;  // luma symbols (P-frames)
    const int16_t* mv;     // int16 [nb][4][3]
    int qp;
    const int32_t* qp_row;
    const int32_t* qp_map;
    int qp_offset;
    int32_t* tokens;       // int32 [2][nb]   (ENC)
    int32_t* sse;          // int32 [2][nb]   (ENC)
};

int chroma_launch(const ChromaArgs& a, bool encode, hipStream_t st);

}  // namespace so
