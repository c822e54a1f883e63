"""CPU restatement of the RCB2 container (TEST INFRASTRUCTURE ONLY; layout and checksum in
include/range_coder.h): build, parse and the per-chunk checksum in numpy, so the GPU's containers
can be compared byte for byte.  The chunk streams inside come from the CPU references
(oracle/cpu.py, order1_ref.py, wide_ref.py); this module only frames them."""
import struct

import numpy as np

HEADER = 64
KIND_STATIC, KIND_ADAPTIVE, KIND_ORDER1, KIND_WIDE = 0, 1, 2, 3
F_CHECKSUMS = 1
GOLD = 0x9E3779B1
M32 = 0xFFFFFFFF


def pad16(v):
    return (v + 15) & ~15


def _pad(b):
    return b + b"\0" * (pad16(len(b)) - len(b))


def fmix32(h):
    """MurmurHash3's 32-bit finaliser on a uint32 array (or an int)."""
    h = np.asarray(h, np.uint64) & M32
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & np.uint64(M32)
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & np.uint64(M32)
    h ^= h >> np.uint64(16)
    return h


def checksum(data):
    """The checksum of one chunk given as bytes (its symbols in chunk order, 16-bit symbols
    little-endian): fmix32(sum_i fmix32(w_i + (i + 1) * GOLD) ^ L), all mod 2^32."""
    b = bytes(data)
    L = len(b)
    w = np.frombuffer(b + b"\0" * (-L % 4), dtype="<u4").astype(np.uint64)
    i = np.arange(1, len(w) + 1, dtype=np.uint64)
    S = int(fmix32((w + i * np.uint64(GOLD)) & np.uint64(M32)).sum()) & M32
    return int(fmix32(S ^ (L & M32)))


def sym_bytes(chunk, kind):
    """A chunk's symbols as the bytes the checksum is taken over."""
    return np.asarray(chunk, "<u2" if kind == KIND_WIDE else np.uint8).tobytes()


def build(kind, n_symbols, chunks, codes, c=None, total=0, adaptive=(0, 0, 0), ctx_map=None,
          first_row=0, checksums=False):
    """chunks: the symbols of every chunk (arrays; uint16 values for kind 3); codes: their
    streams.  c: the table (kinds 0, 3) or the K x n_symbols rows (kind 2)."""
    n = len(chunks)
    p20 = p24 = p28 = 0
    table = b""
    if kind == KIND_ADAPTIVE:
        p20, p24, p28 = adaptive
        total = 0
    elif kind == KIND_ORDER1:
        rows = np.asarray(c, "<u4").reshape(-1, n_symbols)
        p20, p24 = rows.shape[0], first_row
        table = _pad(rows.tobytes() + np.asarray(ctx_map, np.uint8)[:n_symbols].tobytes())
    else:
        table = _pad(np.asarray(c, "<u4").tobytes())
    payload = b"".join(_pad(bytes(cd)) for cd in codes)
    head = b"RCB2" + struct.pack("<IIIIIII", 1 | (HEADER << 16), kind, n_symbols, total, p20, p24,
                                 p28)
    head += struct.pack("<QQQII", n, sum(len(x) for x in chunks), len(payload),
                        F_CHECKSUMS if checksums else 0, 0)
    assert len(head) == HEADER
    index = b"".join(struct.pack("<QQ", len(x), len(cd)) for x, cd in zip(chunks, codes))
    sums = b""
    if checksums:
        sums = _pad(b"".join(struct.pack("<I", checksum(sym_bytes(x, kind))) for x in chunks))
    return head + table + index + sums + payload


def parse(blob):
    """-> dict of the header fields, the section offsets, the table (c rows, ctx_map), the index
    [(symbol count, code bytes)] and the stored checksums (or None)."""
    blob = bytes(blob)
    assert blob[:4] == b"RCB2"
    vh, kind, ns, total, p20, p24, p28 = struct.unpack_from("<IIIIIII", blob, 4)
    n, n_syms, pay, flags, zero = struct.unpack_from("<QQQII", blob, 32)
    d = dict(version=vh & 0xFFFF, header_bytes=vh >> 16, kind=kind, n_symbols=ns,
             total_freq=total, n_chunks=n, n_syms=n_syms, payload_bytes=pay, flags=flags,
             n_models=p20 if kind == KIND_ORDER1 else 0,
             first_row=p24 if kind == KIND_ORDER1 else 0,
             adaptive=(p20, p24, p28) if kind == KIND_ADAPTIVE else (0, 0, 0),
             sym_bytes=2 if kind == KIND_WIDE else 1, table_off=HEADER)
    off = HEADER
    d["c"] = d["ctx_map"] = None
    if kind in (KIND_STATIC, KIND_WIDE):
        d["c"] = np.frombuffer(blob, "<u4", ns, off)
        off += pad16(4 * ns)
    elif kind == KIND_ORDER1:
        d["c"] = np.frombuffer(blob, "<u4", p20 * ns, off).reshape(p20, ns)
        d["ctx_map"] = np.frombuffer(blob, np.uint8, ns, off + 4 * p20 * ns)
        off += pad16(4 * p20 * ns + ns)
    d["index_off"] = off
    idx = [struct.unpack_from("<QQ", blob, off + 16 * k) for k in range(n)]
    off += 16 * n
    d["sum_off"] = off
    d["sums"] = None
    if flags & F_CHECKSUMS:
        d["sums"] = list(struct.unpack_from(f"<{n}I", blob, off))
        off += pad16(4 * n)
    d["payload_off"] = off
    d["container_bytes"] = off + pay
    d["chunks"] = []
    for sc, ln in idx:
        d["chunks"].append((sc, blob[off:off + ln]))
        off += pad16(ln)
    return d
