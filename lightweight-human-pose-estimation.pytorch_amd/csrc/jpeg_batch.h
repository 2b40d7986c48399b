// The host arithmetic of a JPEG batch (jpeg_batch.cpp): the records the JPEG kernels read, where every region of a batch's
// workspace lies, and the filling of the records.  Plain C++ with no HIP include, like jpeg_host.h, so all of it also builds
// with the host compiler alone (tools/jpeg_plan_check.cpp): the kernels trust these offsets without a bounds check.
//
// A workspace is one device allocation [upload][device-only regions].  The upload is built in pinned host memory at the same
// offsets and sent in one copy; record arrays and tables are 16-byte aligned, the end of the upload, the host frames of an
// encode, the device-only regions and the total 256-byte.  Every offset below is in bytes from the workspace's start.
#pragma once
#include <vector>

#include "jpeg_encode_host.h"
#include "jpeg_host.h"

namespace lwp {

// a running offset that hands out regions one behind the other
struct Layout {
    size_t at = 0;
    size_t align(size_t a = 16) { return at = (at + a - 1) / a * a; }
    template <class T> size_t take(size_t n, size_t a = 16) { const size_t o = align(a); at = o + n * sizeof(T); return o; }
};

// ---- the records of the decode (jpeg_kernels.hip): stage A turns the coefficient blocks of a batch into block-padded uint8
// component planes, stage B up-samples, converts and stores BGR
constexpr int kJpegBlocksPerGroup = 32;   // stage A: 8 lanes a block, 256 threads a workgroup
constexpr int kJpegPixelsPerThread = 4;   // stage B: horizontally adjacent output pixels of one thread
constexpr int kJpegUnitsPerGroup = 256;   // stage B: threads (pixel groups) a workgroup
struct JpegPlane {                        // one component of one image
    unsigned block0;                      // its first block in the batch's plane-ordered coefficient array
    int blocks_w;                         // blocks a block row (the plane is blocks_w * 8 bytes wide)
    unsigned qt;                          // uint16 offset of its quantisation table (natural order) in the batch's table array
    unsigned pad_;
    long long plane;                      // byte offset of the plane in the workspace
};
struct JpegImage {
    unsigned unit0;                       // its first pixel group in the batch (a row holds ceil(width / kJpegPixelsPerThread))
    int width, height;
    int mode;                             // 0 grey, 1 4:4:4, 2 4:2:2 (h2v1), 3 4:2:0 (h2v2)
    int chroma_w, chroma_h;               // TRUE size of the chroma planes: the edges the up-sampling replicates
    int stride[3];                        // bytes a row of each plane
    int pad_;
    long long plane[3];                   // byte offsets of the planes in the workspace
    unsigned char* out;                   // height * width * 3 bytes, BGR
};
// ---- of the entropy decode on the device (jpeg_entropy_kernels.hip).  One lane owns one subsequence of
// subseq_bytes bytes of one segment; a workgroup takes kJpegEntropyGroup consecutive subsequences of ONE file.
constexpr int kJpegEntropyGroup = 256;
constexpr int kJpegSubseqDefault = 128;   // bytes; lwp_set_jpeg_entropy's subseq_bytes 0
struct JpegEntFile {
    unsigned seg0, n_segs;                // its segments in the batch's segment array
    unsigned sub0, n_subs;                // its subsequences in the batch's numbering (0: the file is skipped)
    unsigned wg0, n_wgs;                  // its workgroups of the sync and the write pass
    unsigned block0, total_blocks;        // its blocks in the batch's plane-ordered coefficient array
    int components, blocks_per_mcu, mcus_x;
    int h0, v0;                           // sampling of component 0 (the others are 1x1)
    unsigned plane_block[3];              // first block of each plane, file-relative
    int blocks_w[3];
};
struct JpegEntSeg {
    unsigned byte0, n_bytes;              // un-stuffed bytes, byte0 from the start of the batch's byte area
    unsigned first_block, n_blocks;       // stream index (MCU order, file-relative) of its first block; MCUs times blocks per MCU
    unsigned sub0;                        // its first subsequence in the batch's numbering
    unsigned file;
};
// ---- of the encode (jpeg_encode_kernels.hip)
constexpr int kJpegEncBlocksPerGroup = 32;    // stage A: 8 lanes a block, 256 threads a workgroup
constexpr int kJpegEncGroup = 256;            // stages B .. F: threads a workgroup; C and E step over an image in tiles of this many
constexpr int kJpegEncChunk = 32;             // stages E and F: un-stuffed bytes a lane owns
struct JpegEncImage {
    const unsigned char* src;                 // device BGR pixels, width * 3 bytes a row
    long long ubytes, sbytes;                 // byte offsets in the workspace: the un-stuffed scan (zeroed, 32-byte granular), the stuffed scan
    int width, height, hs, vs;                // hs, vs: luma sampling (chroma 1 x 1)
    int mcus_x, mcus_y;
    int blocks_w[3];                          // MCU-padded grid widths
    int real_w[3], real_h[3];                 // blocks that hold samples; the others are dummy blocks
    unsigned block0, n_blocks;                // its blocks in the batch's arrays (coefficients: plane order; bits, offsets: stream order)
    unsigned plane0[3];                       // first block of each plane, image-relative
    unsigned per_mcu, ri_blocks;              // blocks an MCU; blocks a restart interval (0: no restarts)
    unsigned int0, n_int;                     // its restart intervals in the batch's interval array
    unsigned chunk0, n_chunks;                // its chunks (the bound) in the batch's chunk array
    unsigned ucap, scap;                      // bytes available at ubytes and at sbytes
};

// Every function below that can refuse returns JPEG_OK, JPEG_REFUSED (an argument error) or JPEG_CAPACITY and words the
// refusal into msg (kJpegMsg bytes).
constexpr size_t kJpegMsg = 400;

// ---- the one header pass of both decode forms
struct JpegHeaders {
    std::vector<lwp_jpeg_header> hd;      // a refused file's (tolerant calls only): no components, no blocks, no pixels
    std::vector<int> verdict;             // per file: JPEG_OK, or why it takes no part
    uint64_t blocks = 0, units = 0;       // coefficient blocks and pixel groups of the batch
    size_t in_bytes = 0;
    int n_planes = 0;
    int refused = -1;                     // the first refused file, which msg names (a tolerant call carries on behind it)
};
// out: null where the call writes no pixels.  Without `tolerant` the first file that is null or refused ends the pass.
int jpeg_batch_headers(int N, const unsigned char* const* data, const size_t* len, unsigned char* const* out, bool tolerant,
                       JpegHeaders* H, char* msg);

// ---- decode: [upload: coefficients | quantisation tables | plane records | plane starts | image records | image starts]
// [component planes].  In device entropy mode the coefficients are device-only and the upload has more in front (below).
struct JpegDecodePlan {
    size_t coef = 0, qt = 0, planes = 0, pstart = 0, images = 0, istart = 0;
    size_t upload = 0, plane_base = 0, total = 0;
};
void jpeg_decode_plan(const JpegHeaders& H, JpegDecodePlan* P);
// the plane and image records into the staging `host` (P->upload bytes); out: the callers' pixels, or null
void jpeg_decode_fill(const JpegHeaders& H, const JpegDecodePlan& P, unsigned char* const* out, unsigned char* host);

// ---- decode, device entropy: [upload: un-stuffed scans | Huffman tables | quantisation tables | file records | file workgroup
// starts | segment records | segment subsequence starts | the four of the decode][coefficients, status words | subsequence
// records | positions | workgroup entries | workgroup flags | component planes]
struct JpegEntropyPlan {
    JpegDecodePlan d;
    size_t bytes = 0, tab = 0, files = 0, fwg = 0, segs = 0, ssub = 0;
    std::vector<uint64_t> seg_at, byte_at;                // [N + 1] where a file's segments (scan records) and bytes start
    size_t stage_bytes = 0;                               // the upload and, behind it, the [N + 2] status words that come back
    unsigned n_segs = 0, n_subs = 0, n_wgs = 0;           // counted by jpeg_entropy_fill
    size_t status = 0, rec = 0, subpos = 0, wg_entry = 0, wg_dirty = 0;       // placed by jpeg_entropy_place
};
int jpeg_entropy_plan(const JpegHeaders& H, const size_t* len, JpegEntropyPlan* P, char* msg);
// the file and segment records from what jpeg_scan_segments left: scan[seg_at[i] ..] holds n_scan[i] records of file i
int jpeg_entropy_fill(const JpegHeaders& H, JpegEntropyPlan* P, const JpegScanSeg* scan, const size_t* n_scan, int subseq,
                      unsigned char* host, char* msg);
// the second step: the device-only regions for P->n_subs subsequences in P->n_wgs workgroups, and the total
void jpeg_entropy_place(const JpegHeaders& H, JpegEntropyPlan* P);

// ---- encode: [upload: image records | block starts | chunk starts | quantisation tables | Huffman codes | host frames]
// [coefficients | bit counts | bit offsets | interval starts | un-stuffed lengths | stuffed lengths | chunk counts | un-stuffed
// scans | stuffed scans]
struct JpegEncPlan {
    std::vector<JpegEncGeom> geom;
    std::vector<size_t> frame, sbytes;                    // per image: its host frame (mem_host only) and its stuffed scan
    size_t images = 0, bstart = 0, cstart = 0, qt = 0, huff = 0, upload = 0;
    size_t coef = 0, bits = 0, offs = 0, istart = 0, ulen = 0, slen = 0, ffbase = 0, ubytes = 0, ubytes_total = 0, total = 0;
    uint64_t blocks = 0, chunks = 0;
    int restart_interval = 0;
};
int jpeg_enc_plan(int N, const unsigned char* const* frames, bool mem_host, const int* heights, const int* widths, int subsampling,
                  int restart_interval, JpegEncPlan* P, char* msg);
// the records, starts and tables into the staging `host` (P.upload bytes).  dev: the workspace's device address; a host frame
// is copied to its slot and its record points there, a device frame's record holds frames[i] as it is
void jpeg_enc_fill(const JpegEncPlan& P, const unsigned char* const* frames, bool mem_host, const int* heights, const int* widths,
                   int quality, const unsigned char* dev, unsigned char* host);

}  // namespace lwp
