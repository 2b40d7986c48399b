"""A NumPy restatement of the JPEG encoder's forward path (csrc/jpeg_encode_kernels.hip): libjpeg's default
compression path from BGR pixels to quantised coefficients in the project's layout (int16, natural order, plane order,
MCU-padded grids), the fixtures of tests/golden/encjpeg_*.npz (source pixels and the file Pillow wrote of them), and hand-built
AVI / Motion-JPEG containers for the reader.  The restatement is the oracle of test_jpeg_encode_host.py and
test_gpu_jpeg_encode.py; it is itself pinned against the coefficients jpeg_cases.decode_blocks reads from Pillow's files.

Mutation knobs (``mutant``) build deliberately wrong encoders: the tests use them to show that the fixtures would see a bottom
edge padded before the down-sampling, a right edge replicated instead of dummy blocks, a constant down-sampling bias and a
truncating quantiser."""
import glob
import os
import struct

import numpy as np

import jpeg_cases as jc
import jpeg_entropy_cases as jec

GOLDEN = jc.GOLDEN
SAMPLINGS = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}
SHORT = {"4:4:4": "444", "4:2:2": "422", "4:2:0": "420"}      # jpeg_entropy_cases' names
PILLOW = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}                 # Pillow's ``subsampling`` numbers (and the library's)
MUTANTS = ("bottom_before_downsample", "replicate_right", "constant_bias", "truncating_quantiser")

# ITU T.81 Annex K, tables K.1 and K.2, natural order
STD_LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
            18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112,
            100, 103, 99]
STD_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99,
              99] + [99] * 32


def quality_tables(quality):
    """jpeg_quality_scaling and jpeg_add_quant_table with force_baseline: uint16 (4, 64), natural order, slots 0 and 1."""
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    qt = np.zeros((4, 64), dtype=np.uint16)
    for slot, std in enumerate((STD_LUMA, STD_CHROMA)):
        qt[slot] = np.clip((np.array(std, dtype=np.int64) * scale + 50) // 100, 1, 255)
    return qt


def geometry(width, height, sampling):
    """jpeg_entropy_cases.geometry and, as ``real_w`` / ``real_h``, each component's real blocks: ceil(ceil(W h / hmax) / 8)."""
    g = jec.geometry(width, height, SHORT[sampling])
    hs, vs = SAMPLINGS[sampling]
    g["real_w"] = [-(-(-(-width * h // hs)) // 8) for h in g["h_samp"]]
    g["real_h"] = [-(-(-(-height * v // vs)) // 8) for v in g["v_samp"]]
    return g


def _edge(a, rows, cols):
    return np.pad(a, ((0, rows - a.shape[0]), (0, cols - a.shape[1])), mode="edge")


def component_planes(bgr, sampling, mutant=None):
    """The three sample planes, each real_h * 8 by real_w * 8 (with ``replicate_right``: the MCU-padded width), int64."""
    H, W = bgr.shape[:2]
    hs, vs = SAMPLINGS[sampling]
    g = geometry(W, H, sampling)
    b, gr, r = [bgr[:, :, k].astype(np.int64) for k in range(3)]
    y = (19595 * r + 38470 * gr + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * gr + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * gr - 5329 * b + (128 << 16) + 32767) >> 16
    cols = [(g["blocks_w"] if mutant == "replicate_right" else g["real_w"])[c] * 8 for c in range(3)]
    rows = [g["real_h"][c] * 8 for c in range(3)]
    planes = [_edge(y, rows[0], cols[0])]
    for c, p in ((1, cb), (2, cr)):
        if mutant == "bottom_before_downsample":
            p = _edge(p, rows[c] * vs, cols[c] * hs)
        else:
            p = _edge(p, -(-H // vs) * vs, cols[c] * hs)               # the bottom: up to a multiple of vmax rows only
        if (hs, vs) == (2, 1):
            bias = np.arange(cols[c]) & 1
            if mutant == "constant_bias":
                bias = 1
            p = (p[:, 0::2] + p[:, 1::2] + bias) >> 1
        elif (hs, vs) == (2, 2):
            bias = 1 + (np.arange(cols[c]) & 1)
            if mutant == "constant_bias":
                bias = 2
            p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
        planes.append(_edge(p, rows[c], cols[c]))                      # then the down-sampled last row is repeated
    return planes


def _fdct8(x, axis, first):
    """jfdctint.c's 8-point pass along ``axis``: the row pass (``first``) leaves PASS1_BITS of scale, the column pass removes
    them; every DESCALE with its rounding term."""
    d = [np.take(x, k, axis=axis) for k in range(8)]
    t0, t7, t1, t6, t2, t5, t3, t4 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6], d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2

    def descale(v, n):
        return (v + (1 << (n - 1))) >> n
    out = [None] * 8
    if first:
        out[0], out[4] = (t10 + t11) << 2, (t10 - t11) << 2
        n = 11
    else:
        out[0], out[4] = descale(t10 + t11, 2), descale(t10 - t11, 2)
        n = 15
    z1 = (t12 + t13) * 4433
    out[2] = descale(z1 + t13 * 6270, n)
    out[6] = descale(z1 + t12 * -15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    out[7], out[5], out[3], out[1] = descale(t4 + z1 + z3, n), descale(t5 + z2 + z4, n), descale(t6 + z2 + z3, n), descale(t7 + z1 + z4, n)
    return np.stack(out, axis=axis)


def forward_blocks(bgr, sampling, quality, mutant=None):
    """(geometry, coefficients int16 (total_blocks, 64), qtables uint16 (4, 64)) of a BGR uint8 (H, W, 3) frame, laid out as
    jpeg_cases.decode_blocks lays out what it reads from the file."""
    H, W = bgr.shape[:2]
    g = geometry(W, H, sampling)
    qt = quality_tables(quality)
    out = []
    for c, plane in enumerate(component_planes(bgr, sampling, mutant)):
        bh, bw = plane.shape[0] // 8, plane.shape[1] // 8
        blk = (plane - 128).reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)          # [block row][block column][row][column]
        blk = _fdct8(_fdct8(blk, 3, True), 2, False).reshape(bh, bw, 64)         # each row first, then each column
        q8 = 8 * qt[min(c, 1)].astype(np.int64)
        mag = np.abs(blk) // q8 if mutant == "truncating_quantiser" else (np.abs(blk) + (q8 >> 1)) // q8
        real = np.sign(blk) * mag
        grid = np.zeros((g["blocks_h"][c], g["blocks_w"][c], 64), dtype=np.int64)
        grid[:bh, :bw] = real
        hc, vc = g["h_samp"][c], g["v_samp"][c]
        for by in range(g["blocks_h"][c]):                                       # jccoefct.c's compress_data: dummy blocks
            for bx in range(g["blocks_w"][c]):
                if by < bh and bx < bw:
                    continue
                if by < bh:
                    grid[by, bx, 0] = grid[by, bx - 1, 0]                         # right of a real block: its left neighbour's DC
                else:
                    last = (bx // hc) * hc + hc - 1                               # the last block of the row above inside the MCU
                    grid[by, bx, 0] = grid[by - 1, last, 0]
            assert vc <= 2
        out.append(grid.reshape(-1, 64))
    return g, np.concatenate(out).astype(np.int16), qt


def scan_of(coef, g, restart_interval=0, mutant=None, mutant_arg=None):
    """The entropy-coded scan of such coefficients with Annex K's Huffman tables: jpeg_entropy_cases' coder (and its mutants)."""
    return jec.encode_scan(coef, g, jec.standard_tables(), [0, 1, 1], [0, 1, 1], restart_interval, mutant, mutant_arg)


# ---------------------------------------------------------------------------------------------- what a set of coefficients reaches
ALL_AC = frozenset([0x00, 0xF0] + [(r << 4) | s for r in range(16) for s in range(1, 11)])      # Annex K's 162 symbols
ALL_DC = frozenset(range(12))
WORST_BLOCK_BITS = 1658        # luma: 9 + 11 bits of a category-11 DC difference, 63 times a 16-bit code and 10 magnitude bits


def block_symbols(block, pred):
    """(DC category, [AC symbols]) of one block (64 ints, natural order) as jchuff.c's encode_one_block emits them."""
    ac, run = [], 0
    for k in range(1, 64):
        v = block[jec.ZZ[k]]
        if v == 0:
            run += 1
            continue
        ac += [0xF0] * (run >> 4)
        ac.append(((run & 15) << 4) | abs(v).bit_length())
        run = 0
    if run:
        ac.append(0x00)
    return abs(block[0] - pred).bit_length(), ac


def split_scan(scan):
    """The un-stuffed bytes of every restart interval of a stuffed scan, and the RSTn numbers between them."""
    parts, cur, rst, i = [], bytearray(), [], 0
    while i < len(scan):
        b = scan[i]
        if b == 0xFF:
            nxt = scan[i + 1]
            if nxt == 0:
                cur.append(0xFF)
            else:
                assert 0xD0 <= nxt <= 0xD7, "marker %02x inside a scan" % nxt
                parts.append(bytes(cur))
                cur = bytearray()
                rst.append(nxt - 0xD0)
            i += 2
            continue
        cur.append(b)
        i += 1
    parts.append(bytes(cur))
    return parts, rst


def coverage(coef, g, restart=0):
    """What the entropy stages see of these coefficients, from the coefficients, Annex K's code LENGTHS and scan_of's bytes alone
    (never from the library):
      dc, ac            per table (0 luma, 1 chroma): the DC categories coded and the AC symbols emitted (EOB 0x00, ZRL 0xF0)
      max_zrl           the most ZRLs in one gap
      block_bits        the bits of every block, in stream order
      starts            the stream indices at which a restart interval starts (0 first)
      start_bytes       their byte offsets in the un-stuffed scan
      length            the un-stuffed length
      ff                the un-stuffed offsets of the 0xFF bytes; ff_mod32: those modulo 32
      ff_ends           the intervals, the last excepted, whose last byte is 0xFF; ff_last: the scan's last byte is 0xFF
    The two views are held against each other: every interval takes the whole bytes its blocks' bits need."""
    blocks = np.asarray(coef).astype(np.int64).tolist()
    order, comp = jec.stream_order(g)
    per_mcu = len(order) // (g["mcus_x"] * g["mcus_y"])
    tables = jec.standard_tables()
    dc_len = [{s: l for s, (_, l) in jec._codes(*tables[(0, t)]).items()} for t in (0, 1)]
    ac_len = [{s: l for s, (_, l) in jec._codes(*tables[(1, t)]).items()} for t in (0, 1)]
    out = {"dc": [set(), set()], "ac": [set(), set()], "max_zrl": 0, "block_bits": [], "starts": []}
    pred = [0, 0, 0]
    for n, (blk, c) in enumerate(zip(order, comp)):
        if n == 0 or (restart and n % (per_mcu * restart) == 0):
            out["starts"].append(n)
            pred = [0, 0, 0]
        t = min(c, 1)
        cat, syms = block_symbols(blocks[blk], pred[c])
        pred[c] = blocks[blk][0]
        out["dc"][t].add(cat)
        out["ac"][t].update(syms)
        bits, zrl = dc_len[t][cat] + cat, 0
        for s in syms:
            bits += ac_len[t][s] + (s & 15)
            zrl = zrl + 1 if s == 0xF0 else 0
            out["max_zrl"] = max(out["max_zrl"], zrl)
        out["block_bits"].append(bits)
    parts, rst = split_scan(scan_of(coef, g, restart))
    assert len(parts) == len(out["starts"]) and rst == [k & 7 for k in range(len(parts) - 1)]
    ends = out["starts"][1:] + [len(order)]
    for part, a, b in zip(parts, out["starts"], ends):
        assert len(part) == (sum(out["block_bits"][a:b]) + 7) // 8
    flat = b"".join(parts)
    out["start_bytes"] = [0] + np.cumsum([len(p) for p in parts[:-1]]).astype(int).tolist()
    out["length"] = len(flat)
    out["ff"] = [i for i, b in enumerate(flat) if b == 0xFF]
    out["ff_mod32"] = sorted({i % 32 for i in out["ff"]})
    out["ff_ends"] = [k for k, p in enumerate(parts[:-1]) if p[-1] == 0xFF]
    out["ff_last"] = flat[-1] == 0xFF
    return out


# ---------------------------------------------------------------------------------------------- coefficient cases for stages B .. F
def _stream_of(g, c):
    """The plane-order block indices of component c in the order the scan visits them."""
    order, comp = jec.stream_order(g)
    return [b for b, cc in zip(order, comp) if cc == c]


def _place_symbols(coef, blocks, symbols):
    """Writes AC run / size symbols, one behind the other in zig-zag order, into the given (zeroed) blocks; a symbol that no
    longer fits the block opens the next.  Returns the blocks used."""
    used, k = 0, 1
    for sym in sorted(symbols):
        run, size = sym >> 4, sym & 15
        if k + run > 63:
            used, k = used + 1, 1
        coef[blocks[used], jec.ZZ[k + run]] = (1 << size) - 1 if (sym >> 4) & 1 else -(1 << (size - 1))
        k += run + 1
    return used + 1


DC_LADDER = [0, 0, 1, -1, 3, -5, 11, -21, 43, -85, 171, -341, 683]      # the differences: categories 0, 1, 2 .. 11 in turn


def alphabet_case(sampling, width, height, seeds):
    """Random coefficients of several densities (DC differences up to category 11), then hand-placed blocks for what the meter
    says the random part leaves out: every one of Annex K's 160 run / size symbols, EOB and ZRL in both AC tables, and a ladder
    of DC differences through the categories 0 .. 11 at the end of the luma and of the Cb stream."""
    g = geometry(width, height, sampling)
    parts = [jec.random_coefficients(seed, g, density=d, dc=1023) for seed, d in zip(seeds, (1.0, 0.5, 0.2, 0.05, 0.02))]
    coef = parts[0].copy()
    for k, p in enumerate(parts):
        coef[k::len(parts)] = p[k::len(parts)]
    reserve = 28                                       # 160 symbols take 10 * (1 + 2 + .. + 16) = 1360 of 63 places a block
    for c in (0, 1):
        stream = _stream_of(g, c)
        assert len(stream) >= reserve + len(DC_LADDER)
        coef[stream[:reserve], 1:] = 0
    have = coverage(coef, g)
    for c in (0, 1):
        stream = _stream_of(g, c)
        missing = [s for s in ALL_AC - have["ac"][c] if s & 15]
        assert _place_symbols(coef, stream[:reserve - 1], missing) <= reserve - 1
        coef[stream[reserve - 1], 63] = 1             # a gap of 62 zeros: three ZRLs in a row
        coef[stream[-len(DC_LADDER):], 0] = DC_LADDER
    return coef, g


def worst_case(sampling, width, height, restart, all_ones, seed=0):
    """Every block at the luma maximum of WORST_BLOCK_BITS: 63 AC terms of size 10 at run 0 and a DC that alternates between
    -1024 and 1023 along each component's stream, restarting at every interval, so that every difference has category 11.
    ``all_ones``: every magnitude 1023, whose bits are ten ones (the most stuffing); else random magnitudes and signs."""
    g = geometry(width, height, sampling)
    rng = np.random.RandomState(seed)
    n = g["total_blocks"]
    coef = np.full((n, 64), 1023, dtype=np.int64) if all_ones else rng.randint(512, 1024, (n, 64)) * rng.choice([-1, 1], (n, 64))
    order, comp = jec.stream_order(g)
    per_mcu = len(order) // (g["mcus_x"] * g["mcus_y"])
    pred = [0, 0, 0]
    for i, (b, c) in enumerate(zip(order, comp)):
        if restart and i % (per_mcu * restart) == 0:
            pred = [0, 0, 0]
        coef[b, 0] = pred[c] = 1023 if pred[c] == -1024 else -1024
    return coef.astype(np.int16), g


def sparse_case(sampling, width, height, seed):
    """Mixed content at picture-like densities: what the seam cases carry across their tiles."""
    g = geometry(width, height, sampling)
    a = jec.random_coefficients(seed, g, density=0.12, sizes=(1, 7), dc=600)
    b = jec.random_coefficients(seed + 1, g, density=0.6, sizes=(1, 10), dc=1023)
    a[5::7] = b[5::7]
    return a, g


def _search(what, tries, build, accept):
    for seed in range(tries):
        coef, g, restart = build(seed)
        if accept(coverage(coef, g, restart)):
            return coef, g, restart
    raise AssertionError("no %s among %d seeds" % (what, tries))


def ends_in_ff_case(width, restart):
    """A width x 8 4:4:4 image whose scan ends FF 00: the last block (Cr of the last MCU) has a coefficient 63, so it ends in
    magnitude bits and not in EOB; the search runs over the DCs and that coefficient.  With restart 1 an interior interval must
    end in 0xFF too."""
    def build(seed):
        g = geometry(width, 8, "4:4:4")
        rng = np.random.RandomState(1000 + seed)
        coef = np.zeros((g["total_blocks"], 64), dtype=np.int16)
        coef[:, 0] = rng.randint(-1023, 1024, g["total_blocks"])
        coef[2 * g["mcus_x"]:, 63] = rng.randint(1, 1024, g["mcus_x"])          # every Cr block
        return coef, g, restart
    return _search("scan that ends in 0xFF", 200, build, lambda m: m["ff_last"] and (not restart or m["ff_ends"]))


def aligned_start_case():
    """A 48x8 4:4:4 image with restart 1 in which an interval behind the first starts at an un-stuffed offset that is a
    multiple of 32: on the first byte of a chunk of the stuffing passes."""
    def build(seed):
        g = geometry(48, 8, "4:4:4")
        return jec.random_coefficients(2000 + seed, g, density=0.3, sizes=(1, 8), dc=800), g, 1
    return _search("interval start on a chunk boundary", 200, build, lambda m: any(b % 32 == 0 for b in m["start_bytes"][1:]))


_COEF_CASES = None


def coefficient_cases():
    """{name: dict(coef, g, size (H, W), sampling, restart)}: what lwp_debug_jpeg_encode_scan is handed.  Built once."""
    global _COEF_CASES
    if _COEF_CASES is not None:
        return _COEF_CASES
    out = {}

    def add(name, coef, g, sampling, width, height, restart):
        assert coef.dtype == np.int16 and coef.shape == (g["total_blocks"], 64), name
        out[name] = {"coef": np.ascontiguousarray(coef), "g": g, "size": (height, width), "sampling": sampling, "restart": restart}

    for sampling, (w, h), seeds in (("4:2:0", (128, 96), (1, 2, 3, 4, 5)), ("4:4:4", (80, 64), (6, 7, 8, 9, 10))):
        coef, g = alphabet_case(sampling, w, h, seeds)
        add("alphabet_" + SHORT[sampling], coef, g, sampling, w, h, 0)
    for sampling, (w, h) in (("4:2:0", (16, 16)), ("4:4:4", (24, 8))):
        for restart in (0, 1):
            for kind, all_ones in (("random", False), ("ones", True)):
                coef, g = worst_case(sampling, w, h, restart, all_ones, seed=restart)
                add("worst_%s_%s_r%d" % (kind, SHORT[sampling], restart), coef, g, sampling, w, h, restart)
    def seam(sampling, w, h, restart, at, seed0):
        """The interval in front of block ``at`` must leave pad bits, or a lost byte alignment there would not show."""
        def build(seed):
            return sparse_case(sampling, w, h, seed0 + 100 * seed) + (restart,)

        def accept(m):
            k = m["starts"].index(at)
            return sum(m["block_bits"][m["starts"][k - 1]:at]) % 8 != 0
        coef, g, _ = _search("seam with pad bits", 20, build, accept)
        add("tile_seam_%s_r%d" % (SHORT[sampling], restart), coef, g, sampling, w, h, restart)

    for restart in (1, 8, 64):                         # 72 MCUs of 4 blocks: intervals of 4, 32 and 256 blocks
        seam("4:2:2", 144, 64, restart, 256, 40 + restart)
    seam("4:2:0", 256, 144, 128, 768, 50)              # 144 MCUs of 6 blocks: the second interval starts at block 768 = 3 * 256
    for name, (coef, g, restart), w in (("ends_in_ff", ends_in_ff_case(8, 0), 8), ("ends_in_ff_r1", ends_in_ff_case(24, 1), 24),
                                        ("aligned_start_r1", aligned_start_case(), 48)):
        add(name, coef, g, "4:4:4", w, 8, restart)
    for sampling, (w, h) in (("4:4:4", (72, 64)), ("4:2:0", (112, 80))):
        g = geometry(w, h, sampling)
        add("empty_codes_" + SHORT[sampling], np.zeros((g["total_blocks"], 64), dtype=np.int16), g, sampling, w, h, 0)
    _COEF_CASES = out
    return out


_COEF_SCANS = {}


def coefficient_scan(name):
    """scan_of of a coefficient case, computed once per process."""
    if name not in _COEF_SCANS:
        c = coefficient_cases()[name]
        _COEF_SCANS[name] = scan_of(c["coef"], c["g"], c["restart"])
    return _COEF_SCANS[name]


MANY_SIZES = ((1, 1), (7, 7), (8, 9), (17, 23))       # (H, W)


def many_frames(n=300):
    """n small BGR frames of sizes cycling through MANY_SIZES: noise, a ramp with a little noise, and flat colour in turn."""
    rng = np.random.RandomState(77)
    out = []
    for i in range(n):
        h, w = MANY_SIZES[i % len(MANY_SIZES)]
        kind = (i // len(MANY_SIZES)) % 3
        if kind == 0:
            f = rng.randint(0, 256, (h, w, 3))
        elif kind == 1:
            y, x = np.mgrid[0:h, 0:w]
            f = ((3 * x + 2 * y + i) % 200 + 20)[:, :, None] + rng.randint(-4, 5, (h, w, 3))
        else:
            f = np.broadcast_to(rng.randint(0, 256, 3), (h, w, 3))
        out.append(np.ascontiguousarray(f, dtype=np.uint8))
    return out


def limit_frame(height, width):
    """Smooth content for a frame at the dimension limit: a slow ramp along the long side."""
    y, x = np.mgrid[0:height, 0:width]
    v = ((x + y) // 97) % 256
    return np.ascontiguousarray(np.stack([v, 255 - v, (v * 3) % 256], axis=2), dtype=np.uint8)


# ---------------------------------------------------------------------------------------------- fixtures
_FIXTURES = None


def fixtures():
    """{name: dict(bgr, jpeg, quality, sampling, restart)} of every tests/golden/encjpeg_*.npz, loaded once."""
    global _FIXTURES
    if _FIXTURES is None:
        out = {}
        for path in sorted(glob.glob(os.path.join(GOLDEN, "encjpeg_*.npz"))):
            with np.load(path) as z:
                for name in [k[5:] for k in z.files if k.startswith("jpeg/")]:
                    quality, sampling, restart = [int(v) for v in z["opts/" + name]]
                    out[name] = {"bgr": np.ascontiguousarray(z["bgr/" + name]), "jpeg": z["jpeg/" + name].tobytes(), "quality": quality,
                                 "sampling": {v: k for k, v in PILLOW.items()}[sampling], "restart": restart}
        _FIXTURES = out
    return _FIXTURES


_RESTATED = {}


def restated(name):
    """(geometry, coefficients, qtables) of a fixture by the restatement, computed once per process."""
    if name not in _RESTATED:
        f = fixtures()[name]
        _RESTATED[name] = forward_blocks(f["bgr"], f["sampling"], f["quality"])
    return _RESTATED[name]


# ---------------------------------------------------------------------------------------------- containers, from their specification
def dht_segments():
    """Annex K's four tables as the DHT segments a full file carries (DC 0, AC 0, DC 1, AC 1)."""
    t = jec.standard_tables()
    out = b""
    for key in ((0, 0), (1, 0), (0, 1), (1, 1)):
        counts, vals = t[key]
        body = bytes([(key[0] << 4) | key[1]] + list(counts) + list(vals))
        out += b"\xff\xc4" + (len(body) + 2).to_bytes(2, "big") + body
    return out


def strip_dht(data):
    """The file without its DHT segments, as many cameras write their Motion-JPEG frames."""
    data = bytes(data)
    out, pos = bytearray(data[:2]), 2
    while True:
        m = data[pos + 1]
        L = int.from_bytes(data[pos + 2:pos + 4], "big")
        if m != 0xC4:
            out += data[pos:pos + 2 + L]
        pos += 2 + L
        if m == 0xDA:
            return bytes(out) + data[pos:]


def _chunk(fourcc, body):
    return fourcc + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")


def _list(kind, body):
    return b"LIST" + struct.pack("<I", len(body) + 4) + kind + body


def build_avi(frames, width, height, fps=25, handler=b"MJPG", audio=True, rec=True, riff_kind=b"AVI ", video_stream=None):
    """A RIFF AVI written from the container's specification (not by VideoWriter): ``frames`` is a list of JPEG files, b""
    for a dropped frame.  With ``audio`` an ``auds`` stream comes FIRST in the header list (so the video stream is number 1 and
    its chunks are ``01dc``) and a ``00wb`` chunk of odd length stands between the frames; with ``rec`` the first two frames lie
    in a ``LIST rec ``; a JUNK chunk stands in front of the second half.  No idx1: a reader walks ``movi``."""
    vid = 1 if audio else 0
    if video_stream is not None:
        vid = video_stream
    tag = b"%02ddc" % vid
    avih = struct.pack("<14I", 1000000 // fps, 0, 0, 0x10, len(frames), 0, 2 if audio else 1, 0, width, height, 0, 0, 0, 0)
    strh_v = struct.pack("<4s4sIHHIIIIIIII4H", b"vids", handler, 0, 0, 0, 0, 1, fps, 0, len(frames), 0, 0xFFFFFFFF, 0, 0, 0, width, height)
    bih = struct.pack("<IiiHH4sIiiII", 40, width, height, 1, 24, handler, width * height * 3, 0, 0, 0, 0)
    strl_v = _list(b"strl", _chunk(b"strh", strh_v) + _chunk(b"strf", bih))
    strl_a = b""
    if audio:
        strh_a = struct.pack("<4s4sIHHIIIIIIII4H", b"auds", b"\0\0\0\0", 0, 0, 0, 0, 1, 8000, 0, 7, 0, 0xFFFFFFFF, 1, 0, 0, 0, 0)
        wfx = struct.pack("<HHIIHH", 1, 1, 8000, 8000, 1, 8)
        strl_a = _list(b"strl", _chunk(b"strh", strh_a) + _chunk(b"strf", wfx))
    hdrl = _list(b"hdrl", _chunk(b"avih", avih) + strl_a + strl_v)
    chunks = [_chunk(tag, f) for f in frames]
    n_rec = 2 if rec and len(frames) >= 2 else 0
    movi = b""
    if n_rec:
        movi += _list(b"rec ", chunks[0] + (_chunk(b"00wb", b"\x80" * 7) if audio else b"") + chunks[1])
    movi += _chunk(b"JUNK", b"\0" * 5)
    for c in chunks[n_rec:]:
        movi += c
        if audio:
            movi += _chunk(b"00wb", b"\x80" * 3)
    body = riff_kind + hdrl + _list(b"movi", movi)
    return b"RIFF" + struct.pack("<I", len(body)) + body
