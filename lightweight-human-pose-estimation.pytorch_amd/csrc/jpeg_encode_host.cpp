// Host half of the JPEG writer: see jpeg_encode_host.h.  No HIP here.
#include "jpeg_encode_host.h"

#include <cstring>

namespace lwp {
namespace {

const unsigned char kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                   41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                   30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// ITU T.81 Annex K, tables K.1 and K.2, natural order
const unsigned char kStdLuma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,
                                    69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55,  64,
                                    81, 104, 113, 92, 49, 64,  78,  87,  103, 121, 120, 101, 72, 92,  95,  98,  112, 100, 103, 99};
const unsigned char kStdChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                      99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                      99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

// Annex K, tables K.3 .. K.6: codes of length 1..16, then the symbols in code order
struct StdHuff { unsigned char counts[16]; int n; const unsigned char* vals; };
const unsigned char kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const unsigned char kAcLumaVals[162] = {
    1,   2,   3,   0,   4,   17,  5,   18,  33,  49,  65,  6,   19,  81,  97,  7,   34,  113, 20,  50,  129, 145, 161, 8,   35,  66,  177,
    193, 21,  82,  209, 240, 36,  51,  98,  114, 130, 9,   10,  22,  23,  24,  25,  26,  37,  38,  39,  40,  41,  42,  52,  53,  54,  55,
    56,  57,  58,  67,  68,  69,  70,  71,  72,  73,  74,  83,  84,  85,  86,  87,  88,  89,  90,  99,  100, 101, 102, 103, 104, 105, 106,
    115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163,
    164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211,
    212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250};
const unsigned char kAcChromaVals[162] = {
    0,   1,   2,   3,   17,  4,   5,   33,  49,  6,   18,  65,  81,  7,   97,  113, 19,  34,  50,  129, 8,   20,  66,  145, 161, 177, 193,
    9,   35,  51,  82,  240, 21,  98,  114, 209, 10,  22,  36,  52,  225, 37,  241, 23,  24,  25,  26,  38,  39,  40,  41,  42,  53,  54,
    55,  56,  57,  58,  67,  68,  69,  70,  71,  72,  73,  74,  83,  84,  85,  86,  87,  88,  89,  90,  99,  100, 101, 102, 103, 104, 105,
    106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154,
    162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202,
    210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250};
const StdHuff kStd[4] = {                              // in the order of the file's DHT segments: DC 0, AC 0, DC 1, AC 1
    {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, 12, kDcVals},
    {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, 162, kAcLumaVals},
    {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, 12, kDcVals},
    {{0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}, 162, kAcChromaVals}};

struct Out {
    unsigned char* p; size_t n = 0;
    void byte(int v) { p[n++] = (unsigned char)v; }
    void be16(int v) { byte(v >> 8); byte(v & 255); }
    void marker(int m, int body) { byte(0xFF); byte(m); be16(body + 2); }
};

void codes_of(const StdHuff& t, uint32_t* out) {
    unsigned code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        for (int i = 0; i < t.counts[l - 1]; ++i) out[t.vals[k++]] = (code++ << 5) | (unsigned)l;
        code <<= 1;
    }
}

}  // namespace

bool jpeg_enc_geometry(int height, int width, int subsampling, int restart_interval, JpegEncGeom* g) {
    if (height < 1 || height > 65535 || width < 1 || width > 65535 || subsampling < 0 || subsampling > 2 || restart_interval < 0 ||
        restart_interval > 65535)
        return false;
    g->hs = subsampling == 0 ? 1 : 2;
    g->vs = subsampling == 2 ? 2 : 1;
    g->mcus_x = (width + 8 * g->hs - 1) / (8 * g->hs);
    g->mcus_y = (height + 8 * g->vs - 1) / (8 * g->vs);
    g->total_blocks = 0;
    for (int c = 0; c < 3; ++c) {
        const int h = c ? 1 : g->hs, v = c ? 1 : g->vs;
        g->blocks_w[c] = g->mcus_x * h;
        g->blocks_h[c] = g->mcus_y * v;
        g->real_w[c] = ((width * h + g->hs - 1) / g->hs + 7) / 8;
        g->real_h[c] = ((height * v + g->vs - 1) / g->vs + 7) / 8;
        g->total_blocks += (int64_t)g->blocks_w[c] * g->blocks_h[c];
    }
    const int64_t n = (int64_t)g->mcus_x * g->mcus_y;
    g->intervals = restart_interval ? (n + restart_interval - 1) / restart_interval : 1;
    return true;
}

void jpeg_enc_quant_tables(int quality, uint16_t qt[2][64]) {
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;       // jpeg_quality_scaling
    for (int t = 0; t < 2; ++t)
        for (int i = 0; i < 64; ++i) {
            int v = ((t ? kStdChroma[i] : kStdLuma[i]) * scale + 50) / 100;     // jpeg_add_quant_table, force_baseline
            qt[t][i] = (uint16_t)(v < 1 ? 1 : v > 255 ? 255 : v);
        }
}

void jpeg_enc_huffman(JpegEncHuff* t) {
    memset(t, 0, sizeof *t);
    codes_of(kStd[0], t->dc[0]);
    codes_of(kStd[1], t->ac[0]);
    codes_of(kStd[2], t->dc[1]);
    codes_of(kStd[3], t->ac[1]);
}

size_t jpeg_enc_header(int height, int width, int quality, int subsampling, int restart_interval, unsigned char* out) {
    Out o{out};
    uint16_t qt[2][64];
    jpeg_enc_quant_tables(quality, qt);
    o.byte(0xFF); o.byte(0xD8);
    o.marker(0xE0, 14);                                // JFIF 1.1, units 0 (aspect ratio), density 1 x 1, no thumbnail
    for (const char* s = "JFIF"; *s; ++s) o.byte(*s);
    o.byte(0); o.byte(1); o.byte(1); o.byte(0); o.be16(1); o.be16(1); o.byte(0); o.byte(0);
    for (int t = 0; t < 2; ++t) {
        o.marker(0xDB, 65);
        o.byte(t);                                     // 8-bit entries, table t
        for (int i = 0; i < 64; ++i) o.byte(qt[t][kZigzag[i]]);
    }
    o.marker(0xC0, 15);
    o.byte(8); o.be16(height); o.be16(width); o.byte(3);
    const int luma = subsampling == 0 ? 0x11 : subsampling == 1 ? 0x21 : 0x22;
    o.byte(1); o.byte(luma); o.byte(0);
    o.byte(2); o.byte(0x11); o.byte(1);
    o.byte(3); o.byte(0x11); o.byte(1);
    for (int t = 0; t < 4; ++t) {
        o.marker(0xC4, 17 + kStd[t].n);
        o.byte(((t & 1) << 4) | (t >> 1));             // class (0 DC, 1 AC) << 4 | table
        for (int l = 0; l < 16; ++l) o.byte(kStd[t].counts[l]);
        for (int i = 0; i < kStd[t].n; ++i) o.byte(kStd[t].vals[i]);
    }
    if (restart_interval) { o.marker(0xDD, 2); o.be16(restart_interval); }
    o.marker(0xDA, 10);
    o.byte(3); o.byte(1); o.byte(0x00); o.byte(2); o.byte(0x11); o.byte(3); o.byte(0x11);
    o.byte(0); o.byte(63); o.byte(0);
    return o.n;
}

}  // namespace lwp
