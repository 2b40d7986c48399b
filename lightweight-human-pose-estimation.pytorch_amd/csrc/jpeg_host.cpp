// Host half of the JPEG reader: see jpeg_host.h for the scope and the coefficient layout.  No HIP here.
#include "jpeg_host.h"

#include <cstdarg>
#include <cstdio>
#include <cstring>

namespace lwp {
namespace {

const unsigned char kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                   41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                   30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

constexpr int kLookBits = 9;

struct HuffTable {
    bool defined = false;
    unsigned char counts[17] = {0};        // codes of length 1..16
    unsigned char vals[256] = {0};
    int n_vals = 0;
    int maxcode[18];                       // largest code of length l, -1: none
    int valptr[17];                        // index into vals of the first code of length l
    int mincode[17];
    unsigned short look[1 << kLookBits];   // (length << 8) | symbol for codes of up to kLookBits bits, 0: longer
};

struct Parsed {
    lwp_jpeg_header hd;
    uint16_t qt[kJpegQuantSlots][64];
    bool qt_defined[kJpegQuantSlots];
    HuffTable dc[4], ac[4];
    int comp_id[3];
    int td[3], ta[3];
    bool have_sof = false, saw_jfif = false, saw_adobe = false;
    int adobe_transform = 0;
    size_t scan_at = 0;                    // first byte of the entropy-coded data
};

struct Refuse {
    char* msg; size_t cap;
    int operator()(size_t at, const char* fmt, ...) const {
        if (msg && cap) {
            char body[160];
            va_list ap;
            va_start(ap, fmt);
            vsnprintf(body, sizeof body, fmt, ap);
            va_end(ap);
            snprintf(msg, cap, "jpeg: %s (byte %zu)", body, at);
        }
        return JPEG_REFUSED;
    }
};

inline unsigned be16(const unsigned char* p) { return ((unsigned)p[0] << 8) | p[1]; }

// false: the lengths describe no prefix code (more codes of a length than that length has left)
bool build_table(HuffTable& t) {
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        t.valptr[l] = k;
        t.mincode[l] = code;
        if (t.counts[l]) {
            code += t.counts[l];
            if (code > (1 << l)) return false;
            t.maxcode[l] = code - 1;
            k += t.counts[l];
        } else {
            t.maxcode[l] = -1;
        }
        code <<= 1;
    }
    t.maxcode[17] = 0x7fffffff;
    memset(t.look, 0, sizeof t.look);
    for (int l = 1; l <= kLookBits; ++l)
        for (int i = 0; i < t.counts[l]; ++i) {
            const int c = t.mincode[l] + i, sym = t.vals[t.valptr[l] + i];
            const int first = c << (kLookBits - l), n = 1 << (kLookBits - l);
            for (int j = 0; j < n; ++j) t.look[first + j] = (unsigned short)((l << 8) | sym);
        }
    return true;
}

// the Exif orientation of an APP1 payload (1..8), 0 when there is none or the directory is malformed: metadata is reported,
// never a reason to refuse the picture
int exif_orientation(const unsigned char* p, size_t n) {
    if (n < 14 || memcmp(p, "Exif\0\0", 6) != 0) return 0;
    const unsigned char* t = p + 6;
    const size_t tn = n - 6;
    bool le;
    if (t[0] == 'I' && t[1] == 'I') le = true;
    else if (t[0] == 'M' && t[1] == 'M') le = false;
    else return 0;
    auto u16 = [&](size_t o) -> unsigned { return le ? (unsigned)t[o] | ((unsigned)t[o + 1] << 8) : ((unsigned)t[o] << 8) | t[o + 1]; };
    auto u32 = [&](size_t o) -> uint32_t { return le ? (uint32_t)u16(o) | ((uint32_t)u16(o + 2) << 16) : ((uint32_t)u16(o) << 16) | u16(o + 2); };
    if (u16(2) != 42) return 0;
    const uint32_t ifd = u32(4);
    if (ifd > tn || tn - ifd < 2) return 0;
    const unsigned count = u16(ifd);
    for (unsigned i = 0; i < count; ++i) {
        const size_t e = (size_t)ifd + 2 + (size_t)i * 12;
        if (e + 12 > tn) return 0;
        if (u16(e) == 0x0112) {
            if (u16(e + 2) != 3 || u32(e + 4) != 1) return 0;
            const unsigned v = u16(e + 8);
            return v >= 1 && v <= 8 ? (int)v : 0;
        }
    }
    return 0;
}

const char* sof_name(int m) {
    switch (m) {
        case 0xC1: return "SOF1 (extended sequential)";
        case 0xC2: return "SOF2 (progressive)";
        case 0xC3: return "SOF3 (lossless)";
        case 0xC9: case 0xCA: case 0xCB: case 0xCD: case 0xCE: case 0xCF: return "an arithmetic-coded frame";
        default: return "a differential (hierarchical) frame";
    }
}

// reads the marker at pos: any number of 0xFF fill bytes, then the marker byte.  Leaves pos behind it.
int next_marker(const unsigned char* d, size_t len, size_t& pos, int* marker, const Refuse& refuse) {
    if (pos >= len) return refuse(pos, "the stream ends where a marker is expected (truncated)");
    if (d[pos] != 0xFF) return refuse(pos, "expected a marker, found byte 0x%02X", d[pos]);
    while (pos < len && d[pos] == 0xFF) ++pos;
    if (pos >= len) return refuse(pos, "the stream ends inside a marker (truncated)");
    *marker = d[pos++];
    return JPEG_OK;
}

// the payload of the segment whose length field is at pos; leaves pos behind the segment
int segment(const unsigned char* d, size_t len, size_t& pos, const unsigned char** p, size_t* n, const Refuse& refuse) {
    if (len - pos < 2) return refuse(pos, "the stream ends inside a segment length (truncated)");
    const unsigned L = be16(d + pos);
    if (L < 2) return refuse(pos, "a segment length of %u", L);
    if (L > len - pos) return refuse(pos, "a segment length of %u runs past the end of the %zu-byte stream", L, len);
    *p = d + pos + 2;
    *n = L - 2;
    pos += L;
    return JPEG_OK;
}

int read_dqt(Parsed& P, const unsigned char* p, size_t n, size_t at, const Refuse& refuse) {
    if (n == 0) return refuse(at, "an empty DQT segment");
    while (n) {
        const int pq = p[0] >> 4, tq = p[0] & 15;
        if (pq == 1) return refuse(at, "a 16-bit quantisation table (Pq = 1) is out of scope");
        if (pq != 0 || tq > 3) return refuse(at, "a malformed DQT header byte 0x%02X", p[0]);
        if (n < 65) return refuse(at, "a DQT segment too short for its table");
        for (int i = 0; i < 64; ++i) P.qt[tq][kZigzag[i]] = p[1 + i];
        P.qt_defined[tq] = true;
        p += 65; n -= 65;
    }
    return JPEG_OK;
}

int read_dht(Parsed& P, const unsigned char* p, size_t n, size_t at, const Refuse& refuse) {
    if (n == 0) return refuse(at, "an empty DHT segment");
    while (n) {
        const int tc = p[0] >> 4, th = p[0] & 15;
        if (tc > 1 || th > 3) return refuse(at, "a malformed DHT header byte 0x%02X", p[0]);
        if (n < 17) return refuse(at, "a DHT segment too short for its code counts");
        HuffTable& t = tc ? P.ac[th] : P.dc[th];
        int total = 0;
        t.counts[0] = 0;
        for (int l = 1; l <= 16; ++l) { t.counts[l] = p[l]; total += p[l]; }
        if (total > 256 || (size_t)total > n - 17) { t.defined = false; return refuse(at, "a DHT table with %d symbols does not fit its segment", total); }
        memcpy(t.vals, p + 17, (size_t)total);
        t.n_vals = total;
        t.defined = build_table(t);
        if (!t.defined) return refuse(at, "a DHT table whose code lengths describe no prefix code");
        p += 17 + total; n -= 17 + (size_t)total;
    }
    return JPEG_OK;
}

int read_sof(Parsed& P, const unsigned char* p, size_t n, size_t at, const Refuse& refuse) {
    if (P.have_sof) return refuse(at, "a second frame header");
    if (n < 6) return refuse(at, "a frame header too short");
    lwp_jpeg_header& h = P.hd;
    if (p[0] == 12) return refuse(at, "12-bit samples are out of scope");
    if (p[0] != 8) return refuse(at, "a sample precision of %d bits", p[0]);
    h.height = (int)be16(p + 1);
    h.width = (int)be16(p + 3);
    const int nf = p[5];
    if (h.height == 0) return refuse(at, "a height of 0 (defined later by DNL) is out of scope");
    if (h.width == 0) return refuse(at, "a width of 0");
    if (nf == 4) return refuse(at, "4 components (CMYK / YCCK) are out of scope");
    if (nf != 1 && nf != 3) return refuse(at, "%d components", nf);
    if (n != (size_t)6 + 3 * (size_t)nf) return refuse(at, "a frame header whose length does not match its %d components", nf);
    h.components = nf;
    for (int c = 0; c < nf; ++c) {
        const unsigned char* q = p + 6 + 3 * c;
        P.comp_id[c] = q[0];
        h.h_samp[c] = q[1] >> 4;
        h.v_samp[c] = q[1] & 15;
        h.quant_table[c] = q[2];
        if (h.h_samp[c] < 1 || h.h_samp[c] > 4 || h.v_samp[c] < 1 || h.v_samp[c] > 4)
            return refuse(at, "component %d has sampling factors %dx%d", c, h.h_samp[c], h.v_samp[c]);
        if (q[2] > 3) return refuse(at, "component %d names quantisation table %d", c, q[2]);
        for (int e = 0; e < c; ++e)
            if (P.comp_id[e] == P.comp_id[c]) return refuse(at, "two components share the identifier %d", P.comp_id[c]);
    }
    if (nf == 1) {
        h.h_samp[0] = h.v_samp[0] = 1;     // a scan of one component is never interleaved: one block per MCU
    } else {
        const bool luma_ok = (h.h_samp[0] == 1 && h.v_samp[0] == 1) || (h.h_samp[0] == 2 && h.v_samp[0] == 1) || (h.h_samp[0] == 2 && h.v_samp[0] == 2);
        if (!luma_ok || h.h_samp[1] != 1 || h.v_samp[1] != 1 || h.h_samp[2] != 1 || h.v_samp[2] != 1)
            return refuse(at, "sampling %dx%d,%dx%d,%dx%d is out of scope (4:4:4, 4:2:2 and 4:2:0 only)", h.h_samp[0], h.v_samp[0],
                          h.h_samp[1], h.v_samp[1], h.h_samp[2], h.v_samp[2]);
    }
    const int hmax = h.h_samp[0], vmax = h.v_samp[0];
    h.mcus_x = (h.width + 8 * hmax - 1) / (8 * hmax);
    h.mcus_y = (h.height + 8 * vmax - 1) / (8 * vmax);
    h.total_blocks = 0;
    for (int c = 0; c < nf; ++c) {
        h.blocks_w[c] = h.mcus_x * h.h_samp[c];
        h.blocks_h[c] = h.mcus_y * h.v_samp[c];
        h.total_blocks += (int64_t)h.blocks_w[c] * h.blocks_h[c];
    }
    P.have_sof = true;
    return JPEG_OK;
}

int read_sos(Parsed& P, const unsigned char* p, size_t n, size_t at, const Refuse& refuse) {
    if (!P.have_sof) return refuse(at, "a scan in front of the frame header");
    const lwp_jpeg_header& h = P.hd;
    if (n < 1) return refuse(at, "a scan header too short");
    const int ns = p[0];
    if (ns < 1 || ns > 4 || n != (size_t)4 + 2 * (size_t)ns) return refuse(at, "a malformed scan header");
    if (ns != h.components)
        return refuse(at, "a scan of %d of the %d components: several scans (non-interleaved files) are out of scope", ns, h.components);
    for (int c = 0; c < ns; ++c) {
        const int id = p[1 + 2 * c], tab = p[2 + 2 * c];
        if (id != P.comp_id[c]) return refuse(at, "the scan lists component %d where the frame has %d", id, P.comp_id[c]);
        P.td[c] = tab >> 4;
        P.ta[c] = tab & 15;
        if (P.td[c] > 3 || P.ta[c] > 3) return refuse(at, "component %d names Huffman tables %d / %d", c, P.td[c], P.ta[c]);
        if (!P.dc[P.td[c]].defined) return refuse(at, "DC Huffman table %d of component %d is missing", P.td[c], c);
        if (!P.ac[P.ta[c]].defined) return refuse(at, "AC Huffman table %d of component %d is missing", P.ta[c], c);
        if (!P.qt_defined[h.quant_table[c]]) return refuse(at, "quantisation table %d of component %d is missing", h.quant_table[c], c);
    }
    const unsigned char* q = p + 1 + 2 * ns;
    if (q[0] != 0 || q[1] != 63 || q[2] != 0) return refuse(at, "spectral selection %d..%d / approximation 0x%02X in a baseline scan", q[0], q[1], q[2]);
    if (h.components == 3) {
        if (P.saw_adobe && P.adobe_transform != 1)
            return refuse(at, "Adobe colour transform %d (RGB or YCCK data) is out of scope", P.adobe_transform);
        if (!P.saw_adobe && !P.saw_jfif && P.comp_id[0] == 'R' && P.comp_id[1] == 'G' && P.comp_id[2] == 'B')
            return refuse(at, "components named R, G, B without a JFIF or Adobe marker (RGB data) are out of scope");
    }
    return JPEG_OK;
}

int parse(const unsigned char* d, size_t len, Parsed& P, const Refuse& refuse) {
    memset(&P.hd, 0, sizeof P.hd);
    memset(P.qt, 0, sizeof P.qt);
    memset(P.qt_defined, 0, sizeof P.qt_defined);
    if (!d) return refuse(0, "data is null");
    if (len < 4 || d[0] != 0xFF || d[1] != 0xD8) return refuse(0, "no SOI marker: not a JPEG stream");
    size_t pos = 2;
    for (;;) {                                         // every turn consumes at least two bytes
        int m = 0;
        const size_t at = pos;
        int rc = next_marker(d, len, pos, &m, refuse);
        if (rc) return rc;
        if (m == 0xD9) return refuse(at, "EOI in front of any scan");
        if (m == 0xD8) return refuse(at, "a second SOI");
        if (m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) return refuse(at, "marker 0xFF%02X outside a scan", m);
        if (m == 0xC1 || m == 0xC2 || m == 0xC3 || (m >= 0xC5 && m <= 0xC7) || (m >= 0xC9 && m <= 0xCB) || (m >= 0xCD && m <= 0xCF))
            return refuse(at, "%s is out of scope (baseline SOF0 only)", sof_name(m));
        if (m == 0xCC) return refuse(at, "arithmetic coding (DAC) is out of scope");
        if (m == 0xDC) return refuse(at, "DNL is out of scope");
        const unsigned char* p = nullptr;
        size_t n = 0;
        rc = segment(d, len, pos, &p, &n, refuse);
        if (rc) return rc;
        if (m == 0xC0) rc = read_sof(P, p, n, at, refuse);
        else if (m == 0xC4) rc = read_dht(P, p, n, at, refuse);
        else if (m == 0xDB) rc = read_dqt(P, p, n, at, refuse);
        else if (m == 0xDD) {
            if (n != 2) return refuse(at, "a DRI segment of %zu bytes", n + 2);
            P.hd.restart_interval = (int)be16(p);
        } else if (m == 0xDA) {
            rc = read_sos(P, p, n, at, refuse);
            if (rc) return rc;
            P.scan_at = pos;
            return JPEG_OK;
        } else if (m == 0xE0) {
            if (n >= 5 && memcmp(p, "JFIF\0", 5) == 0) P.saw_jfif = true;
        } else if (m == 0xE1) {
            if (P.hd.orientation == 0) P.hd.orientation = exif_orientation(p, n);
        } else if (m == 0xEE) {
            if (n >= 12 && memcmp(p, "Adobe", 5) == 0) { P.saw_adobe = true; P.adobe_transform = p[11]; }
        } else if ((m >= 0xE0 && m <= 0xEF) || m == 0xFE) {
            // APPn / COM: skipped
        } else {
            return refuse(at, "marker 0xFF%02X is out of scope", m);
        }
        if (rc) return rc;
    }
}

// the bit reader of the scan: un-stuffs 0xFF00, stops in front of any marker and never reads past len
struct Bits {
    const unsigned char* d; size_t pos, len;
    uint64_t acc = 0; int n = 0;
    void fill() {
        while (n <= 56) {
            if (pos >= len) return;
            unsigned b = d[pos];
            if (b == 0xFF) {
                if (pos + 1 >= len || d[pos + 1] != 0) return;     // a marker (or the end): nothing more for this interval
                pos += 2;
            } else {
                ++pos;
            }
            acc = (acc << 8) | b;
            n += 8;
        }
    }
    // the next k <= 16 bits, zero-padded past the data
    unsigned peek(int k) const { return (unsigned)(n >= k ? acc >> (n - k) : acc << (k - n)) & ((1u << k) - 1); }
    void drop(int k) { n -= k; }
    void reset() { acc = 0; n = 0; }
};

// one Huffman symbol, -1: the data ended inside the code, -2: the code matches no symbol
inline int decode_symbol(Bits& b, const HuffTable& t) {
    if (b.n < 16) b.fill();
    const unsigned e = t.look[b.peek(kLookBits)];
    if (e) {
        const int l = (int)(e >> 8);
        if (l > b.n) return -1;
        b.drop(l);
        return (int)(e & 255);
    }
    const unsigned v = b.peek(16);
    for (int l = kLookBits + 1; l <= 16; ++l) {
        const int code = (int)(v >> (16 - l));
        if (t.maxcode[l] >= 0 && code <= t.maxcode[l] && code >= t.mincode[l]) {
            if (l > b.n) return -1;
            b.drop(l);
            return t.vals[t.valptr[l] + code - t.mincode[l]];
        }
    }
    return b.n < 16 ? -1 : -2;
}

// s in 1..11 magnitude bits -> the signed value; false: the data ended
inline bool receive_extend(Bits& b, int s, int* out) {
    if (b.n < s) { b.fill(); if (b.n < s) return false; }
    const int v = (int)b.peek(s);
    b.drop(s);
    *out = v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
    return true;
}

}  // namespace

int jpeg_parse_header(const unsigned char* data, size_t len, lwp_jpeg_header* out, char* msg, size_t msg_cap) {
    const Refuse refuse{msg, msg_cap};
    if (!out) return refuse(0, "out is null");
    Parsed P;
    const int rc = parse(data, len, P, refuse);
    *out = P.hd;
    return rc;
}

int jpeg_decode_blocks(const unsigned char* data, size_t len, lwp_jpeg_header* out, int16_t* coef, size_t coef_cap, uint16_t* qtables,
                       char* msg, size_t msg_cap) {
    const Refuse refuse{msg, msg_cap};
    if (!out || !coef || !qtables) return refuse(0, "out / coef / qtables is null");
    Parsed P;
    int rc = parse(data, len, P, refuse);
    *out = P.hd;
    if (rc) return rc;
    const lwp_jpeg_header& h = P.hd;
    // a block takes at least two bits (one DC code, one end-of-block code): a header that promises more blocks than the
    // rest of the stream can hold is refused before anything of that size is touched
    if ((uint64_t)h.total_blocks > 4 * (uint64_t)(len - P.scan_at))
        return refuse(P.scan_at, "the entropy-coded data ends before the last MCU (%lld blocks in %zu bytes)", (long long)h.total_blocks, len - P.scan_at);
    const uint64_t need = 64 * (uint64_t)h.total_blocks;
    if (need > coef_cap) {
        if (msg && msg_cap) snprintf(msg, msg_cap, "jpeg: %llu coefficients do not fit a buffer of %zu", (unsigned long long)need, coef_cap);
        return JPEG_CAPACITY;
    }
    memcpy(qtables, P.qt, sizeof P.qt);
    memset(coef, 0, (size_t)need * sizeof(int16_t));
    int16_t* plane[3] = {coef, nullptr, nullptr};
    for (int c = 1; c < h.components; ++c) plane[c] = plane[c - 1] + (size_t)64 * h.blocks_w[c - 1] * h.blocks_h[c - 1];

    Bits b{data, P.scan_at, len};
    int pred[3] = {0, 0, 0};
    const int64_t n_mcus = (int64_t)h.mcus_x * h.mcus_y;
    int until_restart = h.restart_interval, next_rst = 0;
    int mx = 0, my = 0;
    for (int64_t mcu = 0; mcu < n_mcus; ++mcu) {
        if (h.restart_interval && until_restart == 0) {
            const bool left_over = b.n >= 8;           // whole bytes nobody read; fewer are the padding bits of the interval
            b.reset();
            size_t at = b.pos;
            int m = 0;
            if (left_over || at >= len || data[at] != 0xFF || next_marker(data, len, b.pos, &m, Refuse{nullptr, 0}) || m != 0xD0 + next_rst)
                return refuse(at, "RST%d is missing or wrong in front of MCU %lld", next_rst, (long long)mcu);
            next_rst = (next_rst + 1) & 7;
            until_restart = h.restart_interval;
            pred[0] = pred[1] = pred[2] = 0;
        }
        for (int c = 0; c < h.components; ++c) {
            const HuffTable& dct = P.dc[P.td[c]];
            const HuffTable& act = P.ac[P.ta[c]];
            for (int v = 0; v < h.v_samp[c]; ++v)
                for (int u = 0; u < h.h_samp[c]; ++u) {
                    int16_t* blk = plane[c] + ((size_t)(my * h.v_samp[c] + v) * h.blocks_w[c] + (size_t)(mx * h.h_samp[c] + u)) * 64;
                    int s = decode_symbol(b, dct);
                    if (s == -1) return refuse(b.pos, "the entropy-coded data ends before the last MCU (in MCU %lld of %lld)", (long long)mcu, (long long)n_mcus);
                    if (s == -2) return refuse(b.pos, "a Huffman code that matches no symbol (DC, MCU %lld)", (long long)mcu);
                    if (s > 11) return refuse(b.pos, "a DC category of %d (MCU %lld)", s, (long long)mcu);
                    if (s) {
                        int diff = 0;
                        if (!receive_extend(b, s, &diff)) return refuse(b.pos, "the entropy-coded data ends before the last MCU (in MCU %lld of %lld)", (long long)mcu, (long long)n_mcus);
                        pred[c] += diff;
                        // 8-bit samples give DC values of 11 bits; the bound also keeps the running sum from growing without limit
                        if (pred[c] < -2048 || pred[c] > 2047) return refuse(b.pos, "a DC value of %d is outside 8-bit data's range (MCU %lld)", pred[c], (long long)mcu);
                    }
                    blk[0] = (int16_t)pred[c];
                    for (int k = 1; k < 64;) {
                        const int rs = decode_symbol(b, act);
                        if (rs == -1) return refuse(b.pos, "the entropy-coded data ends before the last MCU (in MCU %lld of %lld)", (long long)mcu, (long long)n_mcus);
                        if (rs == -2) return refuse(b.pos, "a Huffman code that matches no symbol (AC, MCU %lld)", (long long)mcu);
                        const int r = rs >> 4, sz = rs & 15;
                        if (sz == 0) {
                            if (r != 15) break;        // end of block (the run lengths 1..14 with size 0 are read as EOB too, as libjpeg does)
                            k += 16;
                            if (k > 63) return refuse(b.pos, "a zero run pushes the coefficient index past 63 (MCU %lld)", (long long)mcu);
                            continue;
                        }
                        k += r;
                        if (k > 63) return refuse(b.pos, "a zero run pushes the coefficient index past 63 (MCU %lld)", (long long)mcu);
                        if (sz > 10) return refuse(b.pos, "an AC size of %d (MCU %lld)", sz, (long long)mcu);
                        int val = 0;
                        if (!receive_extend(b, sz, &val)) return refuse(b.pos, "the entropy-coded data ends before the last MCU (in MCU %lld of %lld)", (long long)mcu, (long long)n_mcus);
                        blk[kZigzag[k]] = (int16_t)val;
                        ++k;
                    }
                }
        }
        if (h.restart_interval) --until_restart;
        if (++mx == h.mcus_x) { mx = 0; ++my; }
    }
    // behind the last MCU: padding bits, then markers up to EOI.  Whole bytes of entropy data nobody read, another scan, DNL
    // or a stream that just stops are refused
    if (b.n >= 8) return refuse(b.pos, "entropy-coded bytes are left over behind the last MCU");
    size_t pos = b.pos;
    for (;;) {
        int m = 0;
        const size_t at = pos;
        if (pos < len && data[pos] != 0xFF) return refuse(at, "entropy-coded bytes are left over behind the last MCU");
        if (pos >= len) return refuse(at, "the stream ends without EOI (truncated)");
        rc = next_marker(data, len, pos, &m, refuse);
        if (rc) return rc;
        if (m == 0xD9) return JPEG_OK;
        if (m == 0xDA) return refuse(at, "a second scan: several scans are out of scope");
        if (m == 0xDC) return refuse(at, "DNL is out of scope");
        if (m >= 0xD0 && m <= 0xD7) return refuse(at, "RST%d behind the last MCU", m - 0xD0);
        if (m == 0x00 || m == 0x01 || m == 0xD8) return refuse(at, "marker 0xFF%02X behind the scan", m);
        const unsigned char* p = nullptr;
        size_t n = 0;
        rc = segment(data, len, pos, &p, &n, refuse);
        if (rc) return rc;
    }
}

namespace {

void flatten(const HuffTable& t, JpegHuffFlat* f) {
    memset(f, 0, sizeof *f);
    memcpy(f->look, t.look, sizeof f->look);
    for (int l = 1; l <= 16; ++l) { f->maxcode[l] = t.maxcode[l]; f->mincode[l] = t.mincode[l]; f->valptr[l] = t.valptr[l]; }
    f->maxcode[0] = -1;
    memcpy(f->vals, t.vals, sizeof f->vals);
}

}  // namespace

int jpeg_scan_segments(const unsigned char* data, size_t len, const lwp_jpeg_header* hd, unsigned char* bytes, size_t bytes_cap,
                       size_t* n_bytes, JpegScanSeg* segs, size_t segs_cap, size_t* n_segs, JpegHuffFlat* tables, uint16_t* qtables) {
    const Refuse quiet{nullptr, 0};
    if (!data || !hd || !bytes || !n_bytes || !segs || !n_segs || !tables || !qtables) return JPEG_REFUSED;
    *n_bytes = 0; *n_segs = 0;
    Parsed P;
    if (parse(data, len, P, quiet)) return JPEG_REFUSED;
    const lwp_jpeg_header& h = P.hd;
    if (h.width != hd->width || h.height != hd->height || h.components != hd->components || h.h_samp[0] != hd->h_samp[0] ||
        h.v_samp[0] != hd->v_samp[0] || h.restart_interval != hd->restart_interval || h.total_blocks != hd->total_blocks)
        return JPEG_REFUSED;                           // not the file the caller sized its buffers for
    if ((uint64_t)h.total_blocks > 4 * (uint64_t)(len - P.scan_at)) return JPEG_REFUSED;
    memcpy(qtables, P.qt, sizeof P.qt);
    for (int c = 0; c < kJpegHuffPerFile; ++c) memset(&tables[c], 0, sizeof tables[c]);
    for (int c = 0; c < h.components; ++c) { flatten(P.dc[P.td[c]], &tables[c]); flatten(P.ac[P.ta[c]], &tables[3 + c]); }
    const uint64_t n_mcus = (uint64_t)h.mcus_x * (uint64_t)h.mcus_y;
    const size_t expected = jpeg_expected_segments(h);
    if (expected > segs_cap) return JPEG_REFUSED;
    size_t pos = P.scan_at, out = 0, seg_out = 0, n = 0;
    int next_rst = 0;
    auto close_segment = [&]() {
        JpegScanSeg& s = segs[n];
        const uint64_t first = (uint64_t)n * (uint64_t)(h.restart_interval ? h.restart_interval : 0);
        s.byte0 = (uint32_t)seg_out; s.n_bytes = (uint32_t)(out - seg_out);
        s.first_mcu = (uint32_t)first;
        s.n_mcus = (uint32_t)(h.restart_interval ? (n_mcus - first < (uint64_t)h.restart_interval ? n_mcus - first : (uint64_t)h.restart_interval) : n_mcus);
        seg_out = out;
        ++n;
    };
    for (;;) {                                         // every turn moves pos forward
        const void* hit = pos < len ? memchr(data + pos, 0xFF, len - pos) : nullptr;
        const size_t stop = hit ? (size_t)(static_cast<const unsigned char*>(hit) - data) : len;
        const size_t run = stop - pos;
        if (out + run + 1 >= kJpegDeviceScanLimit) return JPEG_CAPACITY;
        if (out + run + 1 > bytes_cap) return JPEG_REFUSED;
        memcpy(bytes + out, data + pos, run);
        out += run; pos = stop;
        if (pos + 1 >= len) return JPEG_REFUSED;       // the stream stops inside the scan or inside a marker: no EOI
        if (data[pos + 1] == 0) { bytes[out++] = 0xFF; pos += 2; continue; }
        size_t q = pos;                                // a marker, fill bytes in front of it allowed
        while (q < len && data[q] == 0xFF) ++q;
        if (q >= len) return JPEG_REFUSED;
        const int m = data[q];
        if (m >= 0xD0 && m <= 0xD7) {
            if (!h.restart_interval || n + 1 >= expected || m != 0xD0 + next_rst) return JPEG_REFUSED;
            close_segment();
            next_rst = (next_rst + 1) & 7;
            pos = q + 1;
            continue;
        }
        close_segment();
        if (n != expected) return JPEG_REFUSED;
        break;
    }
    *n_bytes = out; *n_segs = n;
    // behind the scan: markers up to EOI, as jpeg_decode_blocks walks them
    for (;;) {
        int m = 0;
        if (pos >= len || data[pos] != 0xFF) return JPEG_REFUSED;
        if (next_marker(data, len, pos, &m, quiet)) return JPEG_REFUSED;
        if (m == 0xD9) return JPEG_OK;
        if (m == 0xDA || m == 0xDC || (m >= 0xD0 && m <= 0xD7) || m == 0x00 || m == 0x01 || m == 0xD8) return JPEG_REFUSED;
        const unsigned char* p = nullptr;
        size_t sn = 0;
        if (segment(data, len, pos, &p, &sn, quiet)) return JPEG_REFUSED;
    }
}

}  // namespace lwp
