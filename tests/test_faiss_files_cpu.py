"""include/faiss_files.h on the host: the index file's codec (round trip, hostile files), the directory rules and the ABI.
No device call is made: faiss_file_*, faiss_directory_is_valid and the refusals of the save / load entry points that come
before any HIP call.  Every comparison is an equality of bytes."""
import ctypes as C
import os
import re
import struct
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 1
KINDS = [1, 2, 3]  # IVF-Flat, IVF-PQ, OPQ + IVF-PQ
METRICS = ["L2", "Cosine", "InnerProduct"]
HEADER = 72
OFF_NLIST, OFF_M, OFF_N, OFF_HCRC = 40, 48, 56, 64


def _structure(kind, n, d=32, nlist=4, M=8, d_in=40, seed=0, ids_mode=None):
    """Arbitrary bytes of the right shapes: the codec keeps values as they are."""
    rng = np.random.default_rng(seed + 10 * kind + n)
    s = dict(kind=kind, centroids=rng.standard_normal((nlist, d)).astype(np.float32),
             ids=rng.integers(-2**62, 2**62, n).astype(np.int64), cells=rng.integers(0, nlist, n).astype(np.int32),
             ids_mode=(1 if n else 2) if ids_mode is None else ids_mode)
    if kind == 1:
        s["payload"] = rng.standard_normal((n, d)).astype(np.float16)
    else:
        s["codebooks"] = rng.standard_normal((M, 256, d // M)).astype(np.float32)
        s["payload"] = rng.integers(0, 256, (n, M)).astype(np.uint8)
    if kind == 3:
        s["matrix"] = rng.standard_normal((d, d_in)).astype(np.float32)
    return s


def _write(ff, path, s, metric):
    ff.write_file(path, s["kind"], metric, centroids=s["centroids"], ids_mode=s["ids_mode"], ids=s["ids"], cells=s["cells"],
                  payload=s["payload"], codebooks=s.get("codebooks"), matrix=s.get("matrix"))


def _sections(blob):
    """[(tag, start, end)] of a valid file's sections, 'header' first: start .. end covers head, data and checksum."""
    out = [("header", 0, HEADER)]
    off = HEADER
    while off < len(blob):
        tag = blob[off:off + 4].decode()
        length = struct.unpack_from("<Q", blob, off + 24)[0]
        out.append((tag, off, off + 32 + length + 4))
        off += 32 + length + 4
    assert off == len(blob)
    return out


def _refused(ff, path):
    with pytest.raises(ff.FaissFileError) as e:
        ff.read_file(path)
    assert e.value.code == EINVAL
    return e.value.message


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [70, 0])
def test_codec_round_trip(pkg, tmp_path, kind, metric, n):
    ff = pkg.faiss_files
    m = getattr(pkg.dense_ann.DistanceMetric, metric)
    s = _structure(kind, n)
    path = tmp_path / "x.index"
    _write(ff, path, s, m)
    back = ff.read_file(path, slab=32)  # 70 rows: three slabs, the last one short
    assert (back["kind"], back["metric"], back["n"], back["d"], back["nlist"]) == (kind, m, n, 32, 4)
    assert back["d_in"] == (40 if kind == 3 else 32) and back["M"] == (0 if kind == 1 else 8)
    assert back["ids_mode"] == s["ids_mode"]
    for key in ("centroids", "codebooks", "matrix", "ids", "cells", "payload"):
        assert (key in back) == (key in s)
        if key in s:
            assert back[key].dtype == s[key].dtype and back[key].shape == s[key].shape
            assert back[key].tobytes() == s[key].tobytes(), key
    # the layout faiss_files.h documents: magic, version, then little-endian fields, zlib's CRC-32
    blob = path.read_bytes()
    assert blob[:8] == b"AMDIVFX\0" and struct.unpack_from("<IIII", blob, 8) == (1, kind, int(m), s["ids_mode"])
    assert struct.unpack_from("<QQQQQ", blob, 24) == (back["d_in"], 32, 4, back["M"], n)
    assert struct.unpack_from("<I", blob, OFF_HCRC)[0] == zlib.crc32(blob[:64])
    want = ["header", "CENT"] + ([] if kind == 1 else ["PQCB"]) + (["OPQA"] if kind == 3 else []) + ["RIDS", "CELL"] + ["ROWS" if kind == 1 else "CODE"]
    secs = _sections(blob)
    assert [t for t, _, _ in secs] == want
    for tag, a, b in secs[1:]:
        assert struct.unpack_from("<I", blob, b - 4)[0] == zlib.crc32(blob[a:b - 4]), tag


def test_writer_refuses_shapes_the_reader_would_refuse(pkg, tmp_path):
    ff = pkg.faiss_files
    m = pkg.dense_ann.DistanceMetric.L2
    s = _structure(2, 3)
    s["ids_mode"] = 2  # "no row yet" with three rows
    with pytest.raises(ff.FaissFileError) as e:
        _write(ff, tmp_path / "x", s, m)
    assert e.value.code == EINVAL and "ids mode" in e.value.message
    s = _structure(1, 3, d=24)
    with pytest.raises(ff.FaissFileError):
        _write(ff, tmp_path / "x", s, m)


@pytest.fixture(scope="module")
def smallest(pkg, tmp_path_factory):
    """The smallest valid file of each kind (n = 3, d = 16, nlist = 1, M = 4): {kind: bytes}."""
    ff = pkg.faiss_files
    d = tmp_path_factory.mktemp("smallest")
    out = {}
    for kind in KINDS:
        p = d / f"k{kind}"
        _write(ff, p, _structure(kind, 3, d=16, nlist=1, M=4, d_in=16), pkg.dense_ann.DistanceMetric.Cosine)
        out[kind] = p.read_bytes()
        assert ff.read_file(p)["n"] == 3
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_truncated_at_every_length(pkg, tmp_path, smallest, kind):
    ff = pkg.faiss_files
    blob = smallest[kind]
    path = tmp_path / "t"
    path.write_bytes(blob)
    names = set()
    for size in range(len(blob) - 1, -1, -1):
        os.truncate(path, size)
        msg = _refused(ff, path)
        names.add(msg.split(":")[0])
    # the messages name where the file ended: the header and every section of the kind
    assert "header" in names
    for tag, _, _ in _sections(blob)[1:]:
        assert any(tag in x for x in names), (tag, names)


@pytest.mark.parametrize("kind", KINDS)
def test_a_flipped_bit_in_every_section(pkg, tmp_path, smallest, kind):
    ff = pkg.faiss_files
    blob = smallest[kind]
    path = tmp_path / "f"
    for tag, a, b in _sections(blob):
        # in the section's head (past its tag), in the middle of its data, in its checksum
        places = [a + 12, (a + b) // 2, b - 2] if tag != "header" else [a + 9, a + 20, a + 57, a + 65]
        for at in places:
            bad = bytearray(blob)
            bad[at] ^= 0x10
            path.write_bytes(bytes(bad))
            assert tag in _refused(ff, path), (tag, at)
        if tag != "header":  # the tag itself: the reader names the section it expected there
            bad = bytearray(blob)
            bad[a] ^= 0x01
            path.write_bytes(bytes(bad))
            assert tag in _refused(ff, path)


def _patched(blob, at, value, fix_header_crc):
    bad = bytearray(blob)
    struct.pack_into("<Q", bad, at, value & 0xffffffffffffffff)
    if fix_header_crc:
        struct.pack_into("<I", bad, OFF_HCRC, zlib.crc32(bytes(bad[:64])))
    return bytes(bad)


@pytest.mark.parametrize("kind", KINDS)
def test_huge_and_negative_counts(pkg, tmp_path, smallest, kind):
    """n, M, nlist and a section length replaced by 2^62 and by -1: with the header's checksum left as it was (the checksum
    refuses) and with it made right again (the range checks and the comparison with the file's size refuse)."""
    ff = pkg.faiss_files
    blob = smallest[kind]
    path = tmp_path / "h"
    for value in (1 << 62, -1):
        for at in (OFF_N, OFF_M, OFF_NLIST):
            for fix in (False, True):
                path.write_bytes(_patched(blob, at, value, fix))
                assert "header" in _refused(ff, path)
        for tag, a, _ in _sections(blob)[1:]:
            for field in (8, 16, 24):  # rows, columns, length
                path.write_bytes(_patched(blob, a + field, value, False))
                assert tag in _refused(ff, path)
    # counts that pass the range checks but not the file: n + 1 rows announced, one section longer than the file
    path.write_bytes(_patched(blob, OFF_N, 4, True))
    assert "RIDS" in _refused(ff, path) or "disagrees" in _refused(ff, path)
    tag, a, _ = _sections(blob)[1]
    bad = bytearray(_patched(blob, a + 8, 1 << 20, False))  # rows of CENT
    struct.pack_into("<Q", bad, a + 24, (1 << 20) * 16 * 4)  # a consistent length that overruns the file
    path.write_bytes(bytes(bad))
    assert "CENT" in _refused(ff, path)
    # bytes after the last section
    path.write_bytes(blob + b"\0")
    assert "after the last section" in _refused(ff, path)


@pytest.mark.parametrize("fourcc", [b"IxMp", b"IxM2", b"IxPT", b"IwPQ", b"IwFl"])
def test_native_faiss_files_are_refused_by_name(pkg, tmp_path, smallest, fourcc):
    ff = pkg.faiss_files
    path = tmp_path / "n"
    for body in (fourcc, fourcc + smallest[1][4:], fourcc + bytes(200)):
        path.write_bytes(body)
        assert "native Faiss files are not read" in _refused(ff, path)


def test_wrong_magic_version_and_missing_file(pkg, tmp_path, smallest):
    ff = pkg.faiss_files
    path = tmp_path / "m"
    path.write_bytes(b"NOTANIDX" + smallest[2][8:])
    assert "magic" in _refused(ff, path)
    bad = bytearray(smallest[2])
    struct.pack_into("<I", bad, 8, 2)
    struct.pack_into("<I", bad, OFF_HCRC, zlib.crc32(bytes(bad[:64])))
    path.write_bytes(bytes(bad))
    assert "version" in _refused(ff, path)
    assert "cannot open" in _refused(ff, tmp_path / "absent")
    assert "regular file" in _refused(ff, tmp_path)


def test_directory_rules(pkg, tmp_path, smallest):
    ff = pkg.faiss_files
    lib = ff._lib()
    d = tmp_path / "idx"
    assert not ff.is_valid_faiss_index(d)  # absent
    d.mkdir()
    assert not ff.is_valid_faiss_index(d)
    (d / "_SUCCESS").write_bytes(b"")
    assert not ff.is_valid_faiss_index(d)  # _SUCCESS without faiss.index
    (d / "_SUCCESS").unlink()
    (d / "faiss.index").write_bytes(smallest[2])
    assert not ff.is_valid_faiss_index(d)  # faiss.index without _SUCCESS
    kind, h = C.c_int32(), C.c_void_p()
    assert lib.faiss_index_load_directory(0, os.fsencode(d), 16, 1, C.byref(kind), C.byref(h)) == EINVAL
    assert b"is not an index directory" in lib.faiss_last_error()
    (d / "_SUCCESS").write_bytes(b"")
    assert ff.is_valid_faiss_index(d)
    assert not ff.is_valid_faiss_index(d / "faiss.index")  # a file is not a directory
    # a dimension or a metric that is not the file's is refused before the device is touched
    assert lib.faiss_index_load_directory(0, os.fsencode(d), 32, 1, C.byref(kind), C.byref(h)) == EINVAL
    assert b"dimension 16, not the expected 32" in lib.faiss_last_error()
    assert lib.faiss_index_load_directory(0, os.fsencode(d), 16, 0, C.byref(kind), C.byref(h)) == EINVAL
    assert b"metric" in lib.faiss_last_error()
    # null arguments
    assert lib.faiss_ivf_index_save_directory(None, os.fsencode(d)) == EINVAL
    assert lib.faiss_ivfpq_index_save_directory(None, os.fsencode(d)) == EINVAL
    assert lib.faiss_opq_index_save_directory(None, os.fsencode(d)) == EINVAL
    assert lib.faiss_index_load_directory(0, None, 16, 1, C.byref(kind), C.byref(h)) == EINVAL
    assert lib.faiss_ivf_index_get_rows(None, 0, 0, None) == EINVAL
    assert lib.faiss_index_ids_mode(1, None, None) == EINVAL
    assert lib.faiss_file_close(None) == 0
    with pytest.raises(TypeError):
        ff.write_index(object(), d)


def test_abi_header_protos_and_exports_agree(pkg):
    lib = pkg.load_library()
    header = open(os.path.join(ROOT, "include", "faiss_files.h")).read()
    declared = set(re.findall(r"\b(faiss_[a-z_0-9]+)\s*\(", header))
    assert declared, "no declarations parsed"
    assert declared == set(pkg.faiss_files.PROTOS)
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/faiss_files.h but not exported"
    import subprocess
    syms = subprocess.run(["nm", "-D", "--defined-only", pkg.simclusters_ann.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\b(faiss_[a-z_0-9]+)\b", syms))
    assert exported == declared
