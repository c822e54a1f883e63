"""CPU checks of the RCB2 container (include/range_coder.h): rc_container2_info_parse against the
numpy reference's headers (tests/container2_ref.py), its rejections, the checksum's definition on
known answers and its guarantees, and the Container2Info binding against the header's struct."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest

from range_coder_rust_amd import _native as N

import container2_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "range_coder.h")


def parse2(head):
    inf = N.Container2Info()
    rc = N.load().rc_container2_info_parse(ctypes.c_char_p(bytes(head)), len(head),
                                           ctypes.byref(inf))
    return rc, inf


def sample(kind, checksums, n_chunks=3):
    """A reference container of `kind` with made-up streams (the parse reads the header only)."""
    rng = np.random.default_rng(kind * 2 + checksums)
    codes = [bytes(rng.integers(0, 256, 8 + 5 * k, dtype=np.uint8)) for k in range(n_chunks)]
    if kind == R.KIND_WIDE:
        chunks = [rng.integers(0, 300, 7 + k).astype(np.uint16) for k in range(n_chunks)]
        return R.build(kind, 300, chunks, codes, c=np.full(300, 2), total=600,
                       checksums=checksums)
    chunks = [rng.integers(0, 10, 7 + k).astype(np.uint8) for k in range(n_chunks)]
    if kind == R.KIND_ADAPTIVE:
        return R.build(kind, 10, chunks, codes, adaptive=(32, 57343, 256), checksums=checksums)
    if kind == R.KIND_ORDER1:
        return R.build(kind, 10, chunks, codes, c=np.full((3, 10), 100), total=1000,
                       ctx_map=np.arange(10) % 3, first_row=2, checksums=checksums)
    return R.build(kind, 10, chunks, codes, c=np.full(10, 100), total=1000, checksums=checksums)


@pytest.mark.parametrize("checksums", [False, True])
@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_parse_accepts_the_reference_headers(kind, checksums):
    blob = sample(kind, checksums)
    want = R.parse(blob)
    rc, inf = parse2(blob[:64])
    assert rc == N.RC_OK
    for f in ("version", "kind", "n_symbols", "total_freq", "n_chunks", "n_syms", "payload_bytes",
              "table_off", "index_off", "sum_off", "payload_off", "container_bytes", "flags",
              "n_models", "first_row", "sym_bytes"):
        assert getattr(inf, f) == want[f], f
    assert (inf.increment, inf.limit, inf.period) == want["adaptive"]
    assert inf.container_bytes == len(blob)
    assert bool(inf.flags & N.CONTAINER2_F_CHECKSUMS) == checksums
    # every section starts 16-B aligned
    assert all(getattr(inf, f) % 16 == 0 for f in ("table_off", "index_off", "sum_off",
                                                   "payload_off"))


def test_parse_of_an_empty_container():
    blob = R.build(0, 256, [], [], c=np.full(256, 256), total=65536, checksums=True)
    rc, inf = parse2(blob)
    assert rc == N.RC_OK and inf.n_chunks == 0 and inf.container_bytes == len(blob) == 64 + 1024


def _patched(blob, off, fmt, value):
    b = bytearray(blob[:64])
    struct.pack_into(fmt, b, off, value)
    return bytes(b)


MALFORMED = {
    "magic": (0, 0, "<4s", b"RCB3"),
    "magic_rcb1": (0, 0, "<4s", b"RCB1"),
    "version": (0, 4, "<I", 2 | (64 << 16)),
    "header_size": (0, 4, "<I", 1 | (80 << 16)),
    "kind": (0, 8, "<I", 4),
    "flags": (0, 56, "<I", 2),
    "flags_high": (0, 56, "<I", 1 | (1 << 31)),
    "n_symbols_zero": (0, 12, "<I", 0),
    "n_symbols_257": (0, 12, "<I", 257),
    "n_symbols_257_order1": (2, 12, "<I", 257),
    "n_symbols_4097_wide": (3, 12, "<I", 4097),
    "n_models_zero": (2, 20, "<I", 0),
    "n_models_65": (2, 20, "<I", 65),
    "first_row": (2, 24, "<I", 3),
    "payload_bytes": (0, 48, "<Q", 40),
}


@pytest.mark.parametrize("name", sorted(MALFORMED))
def test_parse_rejects_a_malformed_field(name):
    kind, off, fmt, value = MALFORMED[name]
    blob = sample(kind, True)
    assert parse2(blob[:64])[0] == N.RC_OK
    assert parse2(_patched(blob, off, fmt, value))[0] == N.RC_E_BAD_CONTAINER


def test_parse_bounds_and_arguments():
    blob = sample(0, False)
    assert parse2(blob[:63])[0] == N.RC_E_BAD_CONTAINER
    lib = N.load()
    assert lib.rc_container2_info_parse(None, 64, ctypes.byref(N.Container2Info())) == N.RC_E_ARG
    assert lib.rc_container2_info_parse(ctypes.c_char_p(blob[:64]), 64, None) == N.RC_E_ARG
    # the wide alphabet's range holds for kind 3 only, and 4096 is inside it
    assert parse2(_patched(sample(3, False), 12, "<I", 4096))[0] == N.RC_OK
    assert parse2(_patched(sample(2, False), 20, "<I", 64))[0] == N.RC_OK


def test_rcb1_parse_still_rejects_rcb2_and_the_reverse():
    lib = N.load()
    for kind in range(4):
        blob = sample(kind, True)
        inf = N.ContainerInfo()
        assert lib.rc_container_info_parse(ctypes.c_char_p(blob[:64]), 64,
                                           ctypes.byref(inf)) == N.RC_E_BAD_CONTAINER
    from oracle import container as OC
    rcb1 = OC.build(0, 10, [b"\1\2"], [b"\0" * 9], c=[1] * 10, total=10)
    assert parse2(rcb1[:64])[0] == N.RC_E_BAD_CONTAINER


def test_calls_refuse_an_info_that_parse_did_not_fill():
    """The rc_container2_* calls take their info through a void pointer; a struct without
    parse's mark (an rc_container_info, a zeroed one) is RC_E_ARG before anything is read."""
    lib = N.load()
    inf = N.Container2Info()
    assert lib.rc_container2_offsets(None, None, ctypes.byref(inf), None, None, None) == N.RC_E_ARG
    out = ctypes.c_void_p()
    assert lib.rc_container2_model(None, None, ctypes.byref(inf), ctypes.byref(out)) == N.RC_E_ARG
    bad = ctypes.c_uint64()
    assert lib.rc_container2_verify(None, None, ctypes.byref(inf), None, None,
                                    ctypes.byref(bad)) == N.RC_E_ARG
    assert lib.rc_checksum_batch(None, None, None, 0, 1, None) == N.RC_E_ARG
    size = ctypes.c_uint64()
    assert lib.rc_container2_pack(None, None, None, None, None, None, 0, None, None, 0,
                                  ctypes.byref(size)) == N.RC_E_ARG


def test_status_string_of_the_new_status():
    assert N.RC_E_CHECKSUM == -9
    s = N.status_string(N.RC_E_CHECKSUM)
    assert s and s != "unknown status"
    assert s not in {N.status_string(k) for k in range(-8, 1)}
    consts = dict(re.findall(r"#define (RC_\w+)\s+\(?(-?\d+)u?\)?", open(HEADER).read()))
    assert int(consts["RC_E_CHECKSUM"]) == N.RC_E_CHECKSUM
    assert int(consts["RC_CONTAINER2_F_CHECKSUMS"]) == N.CONTAINER2_F_CHECKSUMS


# ---- the checksum's definition ----

def test_fmix32_known_values():
    # MurmurHash3's finaliser: 0 is its fixed point, fmix32(1) is the familiar 0x514E28B7
    assert int(R.fmix32(0)) == 0
    assert int(R.fmix32(1)) == 0x514E28B7
    assert [int(x) for x in R.fmix32(np.array([0, 1], np.uint32))] == [0, 0x514E28B7]


def test_checksum_hand_computed_values():
    """The definition worked by hand (GOLD = 0x9E3779B1):
    L = 0: no words, S = 0, sum = fmix32(0 ^ 0) = 0.
    L = 1, byte 01: w_0 = 1, S = fmix32(1 + GOLD = 0x9E3779B2) = 0xA64B3DD9,
      sum = fmix32(S ^ 1 = 0xA64B3DD8) = 0xFAFC53D1.
    L = 4, bytes 01 02 03 04: w_0 = 0x04030201, S = fmix32(0xA23A7BB2) = 0x2D9A1727,
      sum = fmix32(S ^ 4 = 0x2D9A1723) = 0xBE44057F.
    L = 5, bytes 01 .. 05: w_0 as before, w_1 = 5 (zero padded), its term
      fmix32(5 + 2 GOLD mod 2^32 = 0x3C6EF367) = 0x5655552B, S = 0x2D9A1727 + 0x5655552B =
      0x83EF6C52, sum = fmix32(S ^ 5 = 0x83EF6C57) = 0x6643D7A4."""
    assert (0x04030201 + R.GOLD) & R.M32 == 0xA23A7BB2 and (5 + 2 * R.GOLD) & R.M32 == 0x3C6EF367
    assert int(R.fmix32(0x9E3779B2)) == 0xA64B3DD9
    assert int(R.fmix32(0xA23A7BB2)) == 0x2D9A1727
    assert int(R.fmix32(0x3C6EF367)) == 0x5655552B
    assert R.checksum(b"") == 0
    assert R.checksum(b"\x01") == 0xFAFC53D1
    assert R.checksum(b"\x01\x02\x03\x04") == 0xBE44057F
    assert R.checksum(b"\x01\x02\x03\x04\x05") == 0x6643D7A4


def test_checksum_of_16_bit_symbols_is_that_of_their_little_endian_bytes():
    assert R.sym_bytes(np.array([0x0201, 0x0403], np.uint16), R.KIND_WIDE) == b"\x01\x02\x03\x04"
    assert R.sym_bytes(np.array([1, 2], np.uint8), R.KIND_STATIC) == b"\x01\x02"


def test_any_single_byte_change_changes_the_checksum():
    """fmix32 is a bijection, so a change confined to one word always changes S: every one of the
    255 other values of every byte of a 37-byte chunk."""
    rng = np.random.default_rng(37)
    base = rng.integers(0, 256, 37, dtype=np.uint8)
    want = R.checksum(base)
    for pos in range(37):
        for delta in range(1, 256):
            b = base.copy()
            b[pos] ^= delta
            assert R.checksum(b) != want, (pos, delta)


def test_length_and_zero_padding_are_told_apart():
    # the same words, different lengths: L enters the last step
    sums = {R.checksum(b"\x07" + b"\0" * k) for k in range(8)}
    assert len(sums) == 8


def test_swapping_two_unequal_words_changes_the_checksum():
    rng = np.random.default_rng(5)
    w = rng.integers(0, 1 << 32, 16, dtype=np.uint64).astype("<u4")
    want = R.checksum(w.tobytes())
    for i in range(16):
        for j in range(i + 1, 16):
            assert w[i] != w[j]
            s = w.copy()
            s[i], s[j] = w[j], w[i]
            assert R.checksum(s.tobytes()) != want, (i, j)


# ---- the binding's struct against the header ----

def test_container2_info_matches_the_header_struct():
    src = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct rc_container2_info \{(.*?)\} rc_container2_info;", src,
                     re.S).group(1)
    width = {"uint32_t": (4, ctypes.c_uint32), "uint64_t": (8, ctypes.c_uint64)}
    fields, off = [], 0
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        typ, names = decl.split(" ", 1)
        size, ct = width[typ]
        for n in names.split(","):
            off = (off + size - 1) // size * size  # natural alignment, as the C compiler lays it
            fields.append((n.strip(), ct, off))
            off += size
    assert [(n, t) for n, t, _ in fields] == list(N.Container2Info._fields_)
    for n, _, o in fields:
        assert getattr(N.Container2Info, n).offset == o, n
    assert ctypes.sizeof(N.Container2Info) == (off + 7) // 8 * 8 == 112
    # rc_container_info's fields come first, unchanged, so the RCB1 struct is a prefix
    assert list(N.Container2Info._fields_[:len(N.ContainerInfo._fields_)]) == \
        list(N.ContainerInfo._fields_)
    assert ctypes.sizeof(N.ContainerInfo) == N.Container2Info.n_models.offset
