// Host half of the JPEG reader (jpeg_host.cpp): marker parse and Huffman decode of baseline files, plain C++ with no HIP
// include, so the file also builds with the host compiler alone (tools/jpeg_host_check.cpp).
//
// In scope: SOF0 (baseline sequential Huffman, 8-bit samples), ONE interleaved scan, 1 component (grey) or 3 (YCbCr), luma
// sampling 1x1 / 2x1 / 2x2 with both chroma components at 1x1, 8-bit quantisation tables, up to 4 + 4 Huffman tables, DRI /
// RSTn, 0xFF fill bytes in front of markers, APPn / COM skipped, APP14 Adobe with transform 1 or no APP14.  Everything else,
// and every malformed or truncated stream, is REFUSED with a message that names the reason and the byte offset; libjpeg warns
// and carries on in several of these cases, this reader does not.
//
// The coefficient interface (what a later device entropy decoder would fill; keep it stable):
//   - int16, 64 per 8x8 block in NATURAL (de-zig-zagged, row-major) order, DC prediction already undone, NOT dequantised;
//   - blocks in PLANE order: component 0's blocks, then component 1's, then component 2's; each component's blocks row-major
//     over its block-padded grid of blocks_w[c] x blocks_h[c] blocks (mcus_x * h_samp[c] by mcus_y * v_samp[c]; the padding
//     blocks of partial MCUs are in the file and are kept);
//   - total_blocks = sum of blocks_w[c] * blocks_h[c]; the image takes 64 * total_blocks coefficients;
//   - the quantisation tables as uint16 in natural order, 4 slots of 64 (a slot the file does not define is zeros);
//     component c uses slot quant_table[c].
// A single-component file is one block per MCU whatever sampling factors its header states (ITU T.81 A.2.2); the header
// reports 1x1 for it.
//
// Every loop is bounded by the input length or the block count and no read leaves [data, data + len).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/lwpose.h"

namespace lwp {

enum { JPEG_OK = 0, JPEG_REFUSED = 1, JPEG_CAPACITY = 2 };

constexpr int kJpegQuantSlots = 4;
constexpr int kJpegHostThreads = 16;                  // lwp_jpeg_decode_batch: threads that share the files of a batch, at most
constexpr size_t kJpegThreadedFromBytes = 256 * 1024; // ... from this many input bytes on; below, one thread (starting them costs more)

// Header only: parses up to and including the first SOS and checks everything that can be checked there.  msg (msg_cap bytes,
// may be null) receives the reason of a refusal.
int jpeg_parse_header(const unsigned char* data, size_t len, lwp_jpeg_header* out, char* msg, size_t msg_cap);

// Header, then the entropy decode of the whole scan into coef (coef_cap int16 available; JPEG_CAPACITY below
// 64 * total_blocks) and the tables into qtables[4 * 64].  On a refusal the contents of coef / qtables are unspecified.
int jpeg_decode_blocks(const unsigned char* data, size_t len, lwp_jpeg_header* out, int16_t* coef, size_t coef_cap,
                       uint16_t* qtables, char* msg, size_t msg_cap);

}  // namespace lwp
