// Host half of the JPEG writer (jpeg_encode_host.cpp): geometry, quality tables, Annex K's Huffman codes and the header bytes
// of the files lwp_jpeg_encode_batch writes.  Plain C++ with no HIP include, like jpeg_host.h.  The layout is Pillow's (libjpeg's
// with a JFIF 1.1 APP0 of density 1 x 1): SOI, APP0, one DQT segment a table, SOF0, four DHT segments, DRI if an interval is set,
// SOS; the scan and EOI follow.
//
// In scope: three components (YCbCr from BGR), 4:4:4 / 4:2:2 (h2v1) / 4:2:0 (h2v2), quality 1..100 through
// jpeg_quality_scaling on Annex K's two quantisation tables (force_baseline: entries clamped to 1..255), Annex K's four Huffman
// tables, a restart interval of 0..65535 MCUs.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace lwp {

struct JpegEncGeom {
    int hs, vs;                            // luma sampling factors (chroma is 1 x 1)
    int mcus_x, mcus_y;
    int blocks_w[3], blocks_h[3];          // the MCU-padded grids: the coefficient layout of jpeg_host.h
    int real_w[3], real_h[3];              // ceil(ceil(W h / hmax) / 8) by ceil(ceil(H v / vmax) / 8): the blocks that hold samples
    int64_t total_blocks;
    int64_t intervals;                     // restart intervals of the scan (1 without restarts)
};

constexpr size_t kJpegEncHeaderMax = 640;  // the header takes 623 bytes, 629 with DRI
// Most bytes the entropy code of one block takes before stuffing: a DC code of up to 11 bits with 11 magnitude bits, 63 AC
// codes of 16 bits with 10 magnitude bits = 1660 bits.
constexpr size_t kJpegEncBlockBytes = 208;

// false: a dimension outside 1..65535, subsampling outside 0..2 or a restart interval outside 0..65535
bool jpeg_enc_geometry(int height, int width, int subsampling, int restart_interval, JpegEncGeom* g);
// bytes the scan takes at most before stuffing (every interval ends on a byte boundary) and after it (every byte stuffed, an
// RSTn marker between intervals)
inline size_t jpeg_enc_unstuffed_bound(const JpegEncGeom& g) { return (size_t)g.total_blocks * kJpegEncBlockBytes + (size_t)g.intervals; }
inline size_t jpeg_enc_scan_bound(const JpegEncGeom& g) { return 2 * jpeg_enc_unstuffed_bound(g) + 2 * (size_t)g.intervals; }
// natural order; slot 0 luminance, slot 1 chrominance
void jpeg_enc_quant_tables(int quality, uint16_t qt[2][64]);
// (code << 5) | length of every symbol of the DC tables [table][category] and the AC tables [table][run << 4 | size];
// 0: the table has no such symbol
struct JpegEncHuff { uint32_t dc[2][16]; uint32_t ac[2][256]; };
void jpeg_enc_huffman(JpegEncHuff* t);
// the header up to and including SOS into out (kJpegEncHeaderMax bytes available); returns its length
size_t jpeg_enc_header(int height, int width, int quality, int subsampling, int restart_interval, unsigned char* out);

}  // namespace lwp
