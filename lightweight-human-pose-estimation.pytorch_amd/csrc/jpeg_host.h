// Host half of the JPEG reader (jpeg_host.cpp): marker parse and Huffman decode of baseline files, plain C++ with no HIP
// include, so the file also builds with the host compiler alone (tools/jpeg_host_check.cpp).
//
// In scope: SOF0 (baseline sequential Huffman, 8-bit samples), ONE interleaved scan, 1 component (grey) or 3 (YCbCr), luma
// sampling 1x1 / 2x1 / 2x2 with both chroma components at 1x1, 8-bit quantisation tables, up to 4 + 4 Huffman tables, DRI /
// RSTn, 0xFF fill bytes in front of markers, APPn / COM skipped, APP14 Adobe with transform 1 or no APP14.  Everything else,
// and every malformed or truncated stream, is REFUSED with a message that names the reason and the byte offset; libjpeg warns
// and carries on in several of these cases, this reader does not.
//
// The coefficient interface (jpeg_decode_blocks fills it on the host, jpeg_entropy_kernels.hip on the device; keep it stable):
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

// ---- The host pre-pass of the DEVICE entropy decoder (jpeg_entropy_kernels.hip).  The kernels fill the coefficient
// layout above from three things this pass leaves: the scan's bytes with every FF 00 reduced to FF, cut at the RSTn markers
// into segments, and the file's Huffman tables flattened.  The pass decodes no symbol; what it cannot see (a code that matches
// nothing, a segment with too few or too many bits, ...) the kernels detect.  It writes no message: jpeg_decode_blocks stays
// the authority for the wording of a refusal and is run on a refused file by the caller.
struct JpegScanSeg {          // one restart interval of the scan
    uint32_t byte0;           // offset of its first un-stuffed byte in the caller's buffer
    uint32_t n_bytes;         // un-stuffed bytes (0: the interval is empty; the kernels refuse it)
    uint32_t first_mcu;       // MCU index of its first MCU
    uint32_t n_mcus;          // restart_interval, fewer in the last
};
struct JpegHuffFlat {         // one Huffman table as the kernels read it: HuffTable's 9-bit look-up and canonical walk
    uint16_t look[512];       // (length << 8) | symbol for codes of up to 9 bits, 0: longer
    int32_t maxcode[17];      // [l]: largest code of length l, -1: none ([0] unused)
    int32_t mincode[17];
    int32_t valptr[17];
    uint8_t vals[256];
    uint8_t pad_[4];
};
static_assert(sizeof(JpegHuffFlat) == 1488 && sizeof(JpegHuffFlat) % 16 == 0, "the kernels copy the table as 16-byte words");
constexpr int kJpegHuffPerFile = 6;                   // DC tables of components 0..2, then their AC tables (a grey file fills [0] and [3])
constexpr size_t kJpegDeviceScanLimit = (size_t)1 << 28;  // un-stuffed bytes of one scan the device mode takes (bit positions are 32-bit)

// how many segments a file with this (accepted) header must have
inline size_t jpeg_expected_segments(const lwp_jpeg_header& h) {
    const uint64_t n = (uint64_t)h.mcus_x * (uint64_t)h.mcus_y;
    return h.restart_interval ? (size_t)((n + (uint64_t)h.restart_interval - 1) / (uint64_t)h.restart_interval) : 1;
}

// One walk over the scan of a file whose header jpeg_parse_header accepted as *hd.  bytes (bytes_cap available; len always
// suffices) receives the un-stuffed entropy-coded bytes of all segments back to back, segs (segs_cap records available;
// jpeg_expected_segments suffices) the segments, tables[kJpegHuffPerFile] and qtables[4 * 64] the tables.  The RST numbering,
// the RST count and the trailer up to EOI are checked as jpeg_decode_blocks checks them.  JPEG_OK: accepted so far;
// JPEG_REFUSED: jpeg_decode_blocks refuses this file too; JPEG_CAPACITY: the un-stuffed scan has kJpegDeviceScanLimit bytes or
// more (the host decoder may well accept it).  Every loop is bounded by len and no read leaves [data, data + len).
int jpeg_scan_segments(const unsigned char* data, size_t len, const lwp_jpeg_header* hd, unsigned char* bytes, size_t bytes_cap,
                       size_t* n_bytes, JpegScanSeg* segs, size_t segs_cap, size_t* n_segs, JpegHuffFlat* tables, uint16_t* qtables);

}  // namespace lwp
