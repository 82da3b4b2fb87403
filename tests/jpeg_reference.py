"""numpy / Python reference of the baseline JPEG decode in csrc/jpeg_decode.hip.

Slow but plain.  ``parse`` reads the markers as ud_jpeg_parse does and builds the same per-component Huffman lookup
(9-bit lookahead + maxcode / valoff slow path); ``decode_coefficients`` is the serial Huffman decode;
``sync_decode_coefficients`` emulates the device's self-synchronising decode (fixed-size subsequences, iterated until
every boundary state agrees) and must give the same coefficients; ``reconstruct`` is libjpeg-turbo's ISLOW IDCT,
fancy upsampling and YCbCr -> RGB, which Pillow runs.
"""
import numpy as np

OK, UNSUPPORTED, TRUNCATED, CORRUPT = 0, 1, 2, 3          # ud_jpeg_parse's UD_JPEG_* codes
LOOKAHEAD = 9

NATURAL = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20,
                    13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52,
                    45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


class JpegError(Exception):
    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


def huff_table(counts, vals):
    """Canonical Huffman code -> (look u16[512]: len << 8 | symbol, 0 = longer than LOOKAHEAD; maxcode i32[18]:
    largest code of each length, -1 if none; valoff i32[18]: index of the first symbol of a length minus its first
    code; vals u8[256])."""
    look = np.zeros(1 << LOOKAHEAD, np.uint16)
    maxcode = np.full(18, -1, np.int32)
    valoff = np.zeros(18, np.int32)
    v = np.zeros(256, np.uint8)
    v[:len(vals)] = vals
    code, k = 0, 0
    for length in range(1, 17):
        n = counts[length - 1]
        if code + n >= (1 << length):             # libjpeg: no all-ones code; before any entry is written
            raise JpegError(CORRUPT, "bad Huffman table")
        if n:
            valoff[length] = k - code
            for _ in range(n):
                if length <= LOOKAHEAD:
                    sh = LOOKAHEAD - length
                    look[code << sh:(code + 1) << sh] = length << 8 | vals[k]
                code += 1
                k += 1
            maxcode[length] = code - 1
        code <<= 1
    return look, maxcode, valoff, v


class Frame:
    pass


def parse(data):
    """-> Frame, or raise JpegError(code).  Mirrors ud_jpeg_parse (csrc/jpeg_decode.hip)."""
    data = bytes(data)
    n = len(data)
    if n < 4 or data[0] != 0xFF or data[1] != 0xD8:
        raise JpegError(CORRUPT, "no SOI")
    pos = 2
    qt, dht, restart, sof, jfif, adobe = {}, {}, 0, None, False, None
    while True:
        if pos + 2 > n:
            raise JpegError(TRUNCATED, "header truncated")
        if data[pos] != 0xFF:
            raise JpegError(CORRUPT, "marker expected")
        while pos < n and data[pos] == 0xFF:
            pos += 1
        if pos >= n:
            raise JpegError(TRUNCATED, "header truncated")
        m = data[pos]
        pos += 1
        if m == 0xD9:
            raise JpegError(TRUNCATED, "EOI before a scan")
        if m in (0xD8, 0x01) or 0xD0 <= m <= 0xD7:
            raise JpegError(CORRUPT, "unexpected marker")
        if pos + 2 > n:
            raise JpegError(TRUNCATED, "header truncated")
        ln = data[pos] << 8 | data[pos + 1]
        if ln < 2:
            raise JpegError(CORRUPT, "bad segment length")
        if pos + ln > n:
            raise JpegError(TRUNCATED, "segment truncated")
        seg = data[pos + 2:pos + ln]
        pos += ln
        if m == 0xE0 and seg[:5] == b"JFIF\0":
            jfif = True
        elif m == 0xEE and len(seg) >= 12 and seg[:5] == b"Adobe":
            adobe = seg[11]
        elif 0xE0 <= m <= 0xEF or m == 0xFE:
            pass
        elif m == 0xDB:
            i = 0
            while i < len(seg):
                pq, tq = seg[i] >> 4, seg[i] & 15
                if pq > 1 or tq > 3:
                    raise JpegError(CORRUPT, "bad DQT")
                w = 64 * (pq + 1)
                if i + 1 + w > len(seg):
                    raise JpegError(CORRUPT, "DQT overruns its segment")
                raw = np.frombuffer(seg[i + 1:i + 1 + w], np.uint8 if pq == 0 else ">u2").astype(np.uint16)
                t = np.zeros(64, np.uint16)
                t[NATURAL] = raw
                qt[tq] = t
                i += 1 + w
        elif m == 0xC4:
            i = 0
            while i < len(seg):
                if i + 17 > len(seg):
                    raise JpegError(CORRUPT, "DHT overruns its segment")
                tc, th = seg[i] >> 4, seg[i] & 15
                counts = list(seg[i + 1:i + 17])
                tot = sum(counts)
                if tc > 1 or th > 3 or tot > 256 or i + 17 + tot > len(seg):
                    raise JpegError(CORRUPT, "bad DHT")
                vals = list(seg[i + 17:i + 17 + tot])
                if tc == 0 and any(v > 15 for v in vals):
                    raise JpegError(CORRUPT, "DC symbol above 15")
                dht[(tc, th)] = huff_table(counts, vals)
                i += 17 + tot
        elif m == 0xDD:
            if len(seg) != 2:
                raise JpegError(CORRUPT, "bad DRI")
            restart = seg[0] << 8 | seg[1]
        elif m in (0xC0, 0xC1):
            if sof is not None:
                raise JpegError(CORRUPT, "second SOF")
            if len(seg) < 6:
                raise JpegError(CORRUPT, "bad SOF")
            prec, H, W, nf = seg[0], seg[1] << 8 | seg[2], seg[3] << 8 | seg[4], seg[5]
            if len(seg) != 6 + 3 * nf:
                raise JpegError(CORRUPT, "bad SOF length")
            if prec != 8 or nf != 3 or H == 0:
                raise JpegError(UNSUPPORTED, "only 8-bit 3-component frames with a height")
            if W == 0:
                raise JpegError(CORRUPT, "zero width")
            sof = (H, W, [(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(3)])
        elif m == 0xDA:
            if sof is None:
                raise JpegError(CORRUPT, "SOS before SOF")
            ns = seg[0] if seg else 0
            if len(seg) != 4 + 2 * ns:
                raise JpegError(CORRUPT, "bad SOS length")
            if ns != 3:
                raise JpegError(UNSUPPORTED, "only one interleaved scan")
            H, W, comps = sof
            if [seg[1 + 2 * c] for c in range(3)] != [c[0] for c in comps]:
                raise JpegError(UNSUPPORTED, "scan components differ from the frame's")
            ss, se, ahal = seg[7], seg[8], seg[9]
            if ss != 0 or se != 63 or ahal != 0:
                raise JpegError(UNSUPPORTED, "not a sequential scan")
            td = [seg[2 + 2 * c] >> 4 for c in range(3)]
            ta = [seg[2 + 2 * c] & 15 for c in range(3)]
            break
        elif m in (0xC2, 0xC3, 0xCC) or 0xC5 <= m <= 0xCF:
            raise JpegError(UNSUPPORTED, f"SOF / DAC marker {m:#x}")
        else:
            raise JpegError(CORRUPT, f"unexpected marker {m:#x}")
    H, W, comps = sof
    hv = [(c[1], c[2]) for c in comps]
    if hv[0] not in ((1, 1), (2, 1), (2, 2)) or hv[1] != (1, 1) or hv[2] != (1, 1):
        raise JpegError(UNSUPPORTED, f"sampling {hv}")
    if adobe == 0 or (adobe is None and not jfif and [c[0] for c in comps] in ([82, 71, 66], [114, 103, 98])):
        raise JpegError(UNSUPPORTED, "RGB colour space")
    for c in range(3):
        if comps[c][3] not in qt or (0, td[c]) not in dht or (1, ta[c]) not in dht:
            raise JpegError(CORRUPT, "table not defined")
    f = Frame()
    f.width, f.height = W, H
    f.hmax, f.vmax = hv[0]
    f.h = [c[1] for c in comps]
    f.v = [c[2] for c in comps]
    f.comp_id = [c[0] for c in comps]
    f.mcus_x = -(-W // (8 * f.hmax))
    f.mcus_y = -(-H // (8 * f.vmax))
    f.bpm = f.hmax * f.vmax + 2
    f.restart = restart
    nmcu = f.mcus_x * f.mcus_y
    f.nseg = -(-nmcu // restart) if restart else 1
    f.cw = [-(-W * f.h[c] // f.hmax) for c in range(3)]
    f.ch = [-(-H * f.v[c] // f.vmax) for c in range(3)]
    f.qt = np.stack([qt[comps[c][3]] for c in range(3)])
    f.huff = [dht[(k, (td if k == 0 else ta)[c])] for c in range(3) for k in (0, 1)]
    # the scan's bytes run to the end of the data; destuff ends the scan at its first marker other than RSTn
    # (normally EOI, bytes after it ignored); without one the scan was cut short and the decode reports the frame
    f.ecs_off, f.ecs_bytes = pos, n - pos
    f.blk_comp = [0] * (f.hmax * f.vmax) + [1, 2]
    return f


# ---- entropy-coded segment ------------------------------------------------------------------------------------
def destuff(data, f):
    """-> list of segments (bytes), FF 00 -> FF and split at RSTn, as k_jd_destuff.  The scan ends at the first other
    marker (or an FF as the last byte).  Raises JpegError(CORRUPT) on a restart number out of order or a segment count
    other than f.nseg."""
    e = bytes(data[f.ecs_off:f.ecs_off + f.ecs_bytes])
    segs, cur, i = [], bytearray(), 0
    while i < len(e):
        b = e[i]
        if b != 0xFF:
            cur.append(b)
            i += 1
            continue
        nxt = e[i + 1] if i + 1 < len(e) else -1
        if nxt == 0:
            cur.append(0xFF)
        elif 0xD0 <= nxt <= 0xD7:
            if nxt - 0xD0 != len(segs) % 8:
                raise JpegError(CORRUPT, "restart marker out of order")
            segs.append(bytes(cur))
            cur = bytearray()
        else:
            break                                       # EOI or another marker: the scan ends here
        i += 2
    segs.append(bytes(cur))
    if len(segs) != f.nseg:
        raise JpegError(CORRUPT, f"{len(segs)} restart segments, expected {f.nseg}")
    return segs


class Bits:
    def __init__(self, seg):
        self.v = int.from_bytes(seg + b"\0\0\0\0\0", "big")   # zeros after the segment, as libjpeg fills
        self.nbits = 8 * len(seg) + 40

    def peek(self, pos, n):
        return (self.v >> (self.nbits - pos - n)) & ((1 << n) - 1) if pos + n <= self.nbits else 0


def _huff(bits, pos, tab):
    """-> (symbol, code length) or (None, 0) for an invalid code."""
    look, maxcode, valoff, vals = tab
    e = int(look[bits.peek(pos, LOOKAHEAD)])
    if e:
        return e & 255, e >> 8
    for length in range(LOOKAHEAD + 1, 17):
        code = bits.peek(pos, length)
        if code <= maxcode[length]:
            return int(vals[valoff[length] + code]), length
    return None, 0


def _extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def step(bits, f, st, sink=None):
    """One symbol (code + extra bits) from state st = (pos, zz, blk).  -> (new state, event): event is None, 'block'
    (a block ended), or 'invalid' (no code matched: the block is abandoned and 16 bits skipped).  sink(zz, value) gets
    the coefficient (the DC difference at zz 0)."""
    pos, zz, blk = st
    c = f.blk_comp[blk]
    if zz == 0:
        s, ln = _huff(bits, pos, f.huff[2 * c])
        if s is None:
            return _next_block(f, pos + 16, blk), "invalid"
        diff = _extend(bits.peek(pos + ln, s), s) if s else 0
        if sink:
            sink(0, diff)
        return (pos + ln + s, 1, blk), None
    rs, ln = _huff(bits, pos, f.huff[2 * c + 1])
    if rs is None:
        return _next_block(f, pos + 16, blk), "invalid"
    r, s = rs >> 4, rs & 15
    pos += ln
    if s:
        zz += r
        if zz > 63:
            return _next_block(f, pos + s, blk), "invalid"
        if sink:
            sink(zz, _extend(bits.peek(pos, s), s))
        zz += 1
        pos += s
    elif r == 15:
        zz += 16
    else:
        zz = 64
    if zz >= 64:
        return _next_block(f, pos, blk), "block"
    return (pos, zz, blk), None


def _next_block(f, pos, blk):
    return (pos, 0, blk + 1 if blk + 1 < f.bpm else 0)


def decode_coefficients(data, f):
    """Serial Huffman decode -> int16 [total_blocks, 64] in natural order (DC predicted), or raise JpegError."""
    segs = destuff(data, f)
    nmcu = f.mcus_x * f.mcus_y
    coef = np.zeros((nmcu * f.bpm, 64), np.int16)
    for si, seg in enumerate(segs):
        bits = Bits(seg)
        b0 = si * f.restart * f.bpm if f.restart else 0
        b1 = min(nmcu, (si + 1) * f.restart if f.restart else nmcu) * f.bpm
        pred = [0, 0, 0]
        st, b = (0, 0, 0), b0
        while b < b1:
            blk = st[2]

            def sink(zz, v, b=b, c=f.blk_comp[blk]):
                if zz == 0:
                    pred[c] += v
                    v = pred[c]
                coef[b, NATURAL[zz]] = np.int16(np.int32(v).astype(np.int16))
            st, ev = step(bits, f, st, sink)
            if ev == "invalid":
                raise JpegError(CORRUPT, "invalid Huffman code")
            if ev == "block":
                b += 1
        if -(-st[0] // 8) != len(seg):
            raise JpegError(CORRUPT, "segment does not end with its last MCU")
    return coef


def sync_decode_coefficients(data, f, sub_bits):
    """The device algorithm: each restart segment is cut into sub_bits-bit subsequences; each subsequence decodes
    from a guessed entry state (its start bit, zz 0, block 0; the first of a segment from the known state) until it
    crosses its end; its exit state becomes the next one's entry, and every subsequence whose entry changed decodes
    again, until no entry changes (at most one round per subsequence).  Block counts and DC sums per subsequence,
    a scan, and a final pass that writes the coefficients.  -> (coef like decode_coefficients, rounds)."""
    segs = destuff(data, f)
    nmcu = f.mcus_x * f.mcus_y
    coef = np.zeros((nmcu * f.bpm, 64), np.int16)
    max_rounds = 0
    for si, seg in enumerate(segs):
        bits = Bits(seg)
        nb = 8 * len(seg)
        nsub = max(1, -(-nb // sub_bits))
        ends = [min((k + 1) * sub_bits, nb) for k in range(nsub)]

        def run(st, end):
            n, dc = 0, [0, 0, 0]

            def sink(zz, v, c):
                if zz == 0:
                    dc[c] += v
            while st[0] < end:
                c = f.blk_comp[st[2]]
                st, ev = step(bits, f, st, lambda zz, v: sink(zz, v, c))
                if ev is not None:
                    n += 1
            return st, n, dc
        X = [run((k * sub_bits, 0, 0) if k else (0, 0, 0), ends[k]) for k in range(nsub)]
        changed = [True] * nsub
        rounds = 1
        for _ in range(nsub):
            nxt = [False] * nsub
            for k in range(1, nsub):
                if changed[k - 1]:
                    r = run(X[k - 1][0], ends[k])
                    nxt[k] = r[0] != X[k][0]
                    X[k] = r
            changed = nxt
            if not any(changed):
                break
            rounds += 1
        max_rounds = max(max_rounds, rounds)
        b0 = si * f.restart * f.bpm if f.restart else 0
        b1 = min(nmcu, (si + 1) * f.restart if f.restart else nmcu) * f.bpm
        base, pred = [b0], [[0, 0, 0]]
        for k in range(nsub - 1):
            base.append(base[-1] + X[k][1])
            pred.append([pred[-1][c] + X[k][2][c] for c in range(3)])
        if base[-1] + X[-1][1] < b1:
            raise JpegError(CORRUPT, "segment decodes fewer blocks than expected")
        for k in range(nsub):
            st = (0, 0, 0) if k == 0 else X[k - 1][0]
            b, p = base[k], list(pred[k])
            while st[0] < ends[k] and b < b1:
                c = f.blk_comp[st[2]]

                def sink(zz, v, b=b, c=c):
                    if zz == 0:
                        p[c] += v
                        v = p[c]
                    coef[b, NATURAL[zz]] = np.int16(np.int32(v).astype(np.int16))
                st, ev = step(bits, f, st, sink)
                if ev == "invalid":
                    raise JpegError(CORRUPT, "invalid Huffman code")
                if ev == "block":
                    b += 1
                    if b == b1 and -(-st[0] // 8) != len(seg):
                        raise JpegError(CORRUPT, "segment does not end with its last MCU")
    return coef, max_rounds


# ---- pixels -----------------------------------------------------------------------------------------------------
def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _idct_1d(s0, s1, s2, s3, s4, s5, s6, s7, out_shift):
    """jidctint.c's butterfly (CONST_BITS 13) on int64 arrays, descaled by out_shift."""
    z1 = (s2 + s6) * 4433
    tmp2 = z1 + s6 * -15137
    tmp3 = z1 + s2 * 6270
    tmp0 = (s0 + s4) << 13
    tmp1 = (s0 - s4) << 13
    t10, t13, t11, t12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    t0, t1, t2, t3 = s7, s5, s3, s1
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * 9633
    t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    t0 += z1 + z3
    t1 += z2 + z4
    t2 += z2 + z3
    t3 += z1 + z4
    d = lambda x: _descale(x, out_shift)
    return [d(t10 + t3), d(t11 + t2), d(t12 + t1), d(t13 + t0), d(t13 - t0), d(t12 - t1), d(t11 - t2), d(t10 - t3)]


def idct_islow(coef, q):
    """Dequantise + ISLOW IDCT of blocks coef int [n, 64] (natural order) with q [64] -> uint8 [n, 8, 8].  The final
    range limit is a clamp, as libjpeg-turbo's SIMD IDCT (packsswb) does, not the C code's masked table."""
    c = coef.astype(np.int64) * q.astype(np.int64)
    c = c.reshape(-1, 8, 8)                                # [n][row v][col u]
    ws = np.stack(_idct_1d(*[c[:, k, :] for k in range(8)], 11), 1)       # columns: pass 1, PASS1_BITS 2
    out = np.stack(_idct_1d(*[ws[:, :, k] for k in range(8)], 18), 2)     # rows: pass 2, + 3 for the 8x8 scaling
    return np.clip(out + 128, 0, 255).astype(np.uint8)


def planes(coef, f):
    """IDCT every block into its component plane: list of uint8 [mcus_y*v*8, mcus_x*h*8]."""
    out = []
    blocks = coef.reshape(f.mcus_y, f.mcus_x, f.bpm, 64)
    j0 = 0
    for c in range(3):
        h, v = f.h[c], f.v[c]
        b = blocks[:, :, j0:j0 + h * v].reshape(-1, 64)
        j0 += h * v
        px = idct_islow(b, f.qt[c]).reshape(f.mcus_y, f.mcus_x, v, h, 8, 8)
        out.append(px.transpose(0, 2, 4, 1, 3, 5).reshape(f.mcus_y * v * 8, f.mcus_x * h * 8))
    return out


def upsample(p, f, c):
    """libjpeg's upsampling of component plane p to the luma grid [H, W] (int64): fancy h2v1 / h2v2 (triangle filter,
    alternating rounding biases, edges replicated), or box when the downsampled width is 2 or less."""
    H, W = f.height, f.width
    cw, ch = f.cw[c], f.ch[c]
    a = p[:ch, :cw].astype(np.int64)
    hs, vs = f.hmax // f.h[c], f.vmax // f.v[c]
    if hs == 1 and vs == 1:
        return a[:H, :W]
    if cw <= 2:
        return np.repeat(np.repeat(a, vs, 0), hs, 1)[:H, :W]
    if vs == 2:
        up = np.concatenate([a[:1], a[:-1]], 0)
        dn = np.concatenate([a[1:], a[-1:]], 0)
        cs = np.empty((2 * ch, cw), np.int64)
        cs[0::2] = 3 * a + up
        cs[1::2] = 3 * a + dn
        lb, rb, sh = 8, 7, 4
    else:
        cs, lb, rb, sh = a, 1, 2, 2
    left = np.concatenate([cs[:, :1], cs[:, :-1]], 1)
    right = np.concatenate([cs[:, 1:], cs[:, -1:]], 1)
    out = np.empty((cs.shape[0], 2 * cw), np.int64)
    out[:, 0::2] = (3 * cs + left + lb) >> sh
    out[:, 1::2] = (3 * cs + right + rb) >> sh
    return out[:H, :W]


def ycc_to_rgb(y, cb, cr):
    """jdcolor.c ycc_rgb_convert: SCALEBITS 16 fixed-point tables, ONE_HALF rounding."""
    fix = lambda x: int(x * 65536 + 0.5)
    cb, cr = cb - 128, cr - 128
    r = y + ((fix(1.40200) * cr + 32768) >> 16)
    g = y + ((-fix(0.34414) * cb + -fix(0.71414) * cr + 32768) >> 16)
    b = y + ((fix(1.77200) * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def reconstruct(coef, f):
    p = planes(coef, f)
    y = p[0][:f.height, :f.width].astype(np.int64)
    return ycc_to_rgb(y, upsample(p[1], f, 1), upsample(p[2], f, 2))


def decode(data):
    """Full reference decode -> uint8 [H, W, 3]; raises JpegError."""
    f = parse(data)
    return reconstruct(decode_coefficients(data, f), f)
