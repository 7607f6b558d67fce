"""`vrag_chunk_markdown` (csrc/chunk.hip) record for record against tests/chunk_ref.py, the restatement of rules R1-R8 that
tests/test_chunker_host.py pins to the reference's own chunker.  Both tables and doc_chunk_off are compared exactly, for every
document of every call; nothing is sampled."""
import ctypes as C
import json
import os
import random
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import chunk_ref  # noqa: E402

ALPHABET = ["#", " ", "\n", "\t", "a", "b", "|", "`", "\r", "\u00a0", "\u3000", "é", "😀", "\x0b", "\x1c", "\u0085", "-"]
WEIGHTS = [6, 4, 5, 1, 3, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1]
CONFIGS = [((1, 2, 3, 4), True), ((2, 3), False), ((1, 2, 3, 4, 5, 6), True)]
OK, INVALID, CAPACITY, NO_DEVICE = 0, -1, -3, -4


def mask_of(levels):
    return sum(1 << l for l in levels)


def call(blobs, levels, preamble, header_cap=None, chunk_cap=None, device=0):
    """(status, headers, chunks, doc_chunk_off, n_headers, n_chunks) of one raw call; caps default to the wrapper's host bound."""
    from verbatim_rag_amd import _lib

    lib = _lib.load()
    off = np.zeros(len(blobs) + 1, np.int64)
    np.cumsum([len(b) for b in blobs], out=off[1:])
    if header_cap is None:
        header_cap = sum(b.count(b"\n#") + 1 for b in blobs)
    if chunk_cap is None:
        chunk_cap = header_cap + len(blobs)
    headers = np.full((max(header_cap, 1), 8), -7, np.int32)
    chunks = np.full((max(chunk_cap, 1), 10), -7, np.int32)
    dco = np.full(len(blobs) + 1, -7, np.int64)
    nh, nc = C.c_int64(-7), C.c_int64(-7)
    blob = b"".join(blobs) or b"\x00"
    buf = (C.c_char * len(blob)).from_buffer_copy(blob)
    st = lib.vrag_chunk_markdown(C.cast(buf, C.c_void_p), off.ctypes.data_as(C.POINTER(C.c_int64)), len(blobs), mask_of(levels),
                                 int(preamble), header_cap, headers.ctypes.data_as(C.c_void_p), chunk_cap,
                                 chunks.ctypes.data_as(C.c_void_p), C.byref(nh), C.byref(nc), dco.ctypes.data_as(C.POINTER(C.c_int64)), device)
    return st, headers, chunks, dco, nh.value, nc.value


def expected(blobs, levels, preamble):
    headers, chunks, dco = [], [], [0]
    for d, b in enumerate(blobs):
        h, c = chunk_ref.tables(b, levels, preamble, doc=d, header_base=len(headers))
        headers += h
        chunks += c
        dco.append(len(chunks))
    return headers, chunks, dco


def check(blobs, levels, preamble):
    st, headers, chunks, dco, nh, nc = call(blobs, levels, preamble)
    assert st == OK
    want_h, want_c, want_off = expected(blobs, levels, preamble)
    assert (nh, nc) == (len(want_h), len(want_c))
    assert dco.tolist() == want_off
    got_h, got_c = headers[:nh].tolist(), chunks[:nc].tolist()
    if got_h != want_h:
        i = next(i for i, (a, b) in enumerate(zip(got_h, want_h)) if a != b)
        d = want_h[i][0]
        raise AssertionError(f"header {i}: got {got_h[i]}, want {want_h[i]}; document {d} = {blobs[d][:80]!r} ({len(blobs[d])} bytes)")
    if got_c != want_c:
        i = next(i for i, (a, b) in enumerate(zip(got_c, want_c)) if a != b)
        d = want_c[i][0]
        raise AssertionError(f"chunk {i}: got {got_c[i]}, want {want_c[i]}; document {d} = {blobs[d][:80]!r} ({len(blobs[d])} bytes)")
    return nh, nc


def test_every_fixture_text():
    with open(os.path.join(HERE, "golden", "chunker_fixtures.json")) as f:
        cases = json.load(f)["chunker"]
    texts = list(dict.fromkeys(c["text"] for c in cases))
    assert len(texts) > 200
    blobs = [chunk_ref.encode(t) for t in texts]
    for levels, preamble in CONFIGS + [((1, 2, 3, 4), False), ((6,), True), ((), True)]:
        check(blobs, levels, preamble)
        for b in blobs[:40]:                                   # and one document per call
            check([b], levels, preamble)


def test_two_thousand_random_documents_in_one_call():
    rng = random.Random(77)
    texts = ["".join(rng.choices(ALPHABET, WEIGHTS, k=rng.randrange(0, 65))) for _ in range(2000)]
    blobs = [chunk_ref.encode(t) for t in texts]
    blobs = [b""] * 3 + blobs[:700] + [b""] * 5 + blobs[700:1400] + [b""] + blobs[1400:] + [b""] * 2   # empty first, last, in runs
    total = 0
    for levels, preamble in CONFIGS:
        total += check(blobs, levels, preamble)[0]
    assert total > 3000                                        # the alphabet makes headers, not just text
    check([b"", b"", b""], (1, 2, 3, 4), True)                 # nothing but empty documents: no byte to scan at all


PATTERNS = ["\n###### x", "\n#\u3000x", "\n#\n\n\nx\n", "\n####### x", "é\n# x"]


def sweep_documents():
    docs = []
    for shift in range(6, 15):                                 # B = 64 .. 16384
        B = 1 << shift
        for pat in PATTERNS:
            p = pat.encode("utf-8")
            for at in range(B - 8, B + 9):
                doc = bytearray(b"ab" * ((B + 64) // 2))
                doc[at:at + len(p)] = p
                docs.append((B, bytes(doc)))
    return docs


def test_boundary_sweep_across_lane_and_workgroup_slices():
    """A '#' run, the white-space character behind it and a '\\n' straddling the 16-byte slice of a lane and the 4 KiB slice of a
    workgroup: each pattern slides over B - 8 .. B + 8 in a document that starts at a multiple of max(B, 4096) in the batch
    (filler documents in between), then again with every document one byte further (odd offsets)."""
    docs = sweep_documents()
    assert len(docs) == 9 * 5 * 17
    for lead in (0, 1):
        blobs, size = [], 0
        for B, doc in docs:
            align = max(B, 4096)
            pad = (lead - size) % align
            blobs.append((b"ab" * (pad // 2 + 1))[:pad - 1] + b"\n" if pad else b"")   # the filler ends a line: the document starts one anyway
            blobs.append(doc)
            assert (size + pad) % align == lead
            size += pad + len(doc)
        nh, _ = check(blobs, (1, 2, 3, 4, 5, 6), True)
        assert nh == 9 * 4 * 17                                # every pattern but the seven hashes is one header
    check([d for _, d in docs], (1, 2, 3, 4), False)           # and back to back, no filler


def test_one_document_of_100k_headers():
    """Large counts, a long pop sequence, doc_chunk_off: 100 000 one-line headers that climb to level 6 and fall back."""
    cycle = [1, 2, 3, 4, 5, 6, 5, 4, 3, 2]
    big = "".join(f"{'#' * cycle[i % 10]} h{i}\n" for i in range(100_000)).encode()
    blobs = [b"intro\n# a\n", big, b"", b"## tail\nx"]
    nh, nc = check(blobs, (1, 2, 3, 4, 5, 6), True)
    assert (nh, nc) == (100_002, 100_004)
    nh, nc = check(blobs, (2, 5), False)
    assert nh == 100_002 and nc == 40_000 + 1 + 1              # levels 2 and 5: four lines of every ten; the empty document; the tail


def test_capacity_path_reports_the_exact_needs():
    blobs = [b"pre\n# a\n## b\n", b"", b"# c\n##### d\n# e"]
    want_h, want_c, want_off = expected(blobs, (1, 2), True)
    assert (len(want_h), len(want_c)) == (5, 6)
    for hcap, ccap in ((4, 6), (5, 5), (0, 0)):
        st, _, chunks, dco, nh, nc = call(blobs, (1, 2), True, hcap, ccap)
        assert st == CAPACITY and (nh, nc) == (5, 6) and dco.tolist() == want_off
        assert (chunks == -7).all()                            # nothing is written when it does not all fit
    st, headers, chunks, dco, nh, nc = call(blobs, (1, 2), True, 5, 6)
    assert st == OK and headers[:5].tolist() == want_h and chunks[:6].tolist() == want_c


def test_argument_errors():
    from verbatim_rag_amd import _lib

    blobs = [b"# a\nb\n"]
    assert call(blobs, (0,), True)[0] == INVALID and "split_levels" in _lib.last_error()
    assert call(blobs, (7,), True)[0] == INVALID
    assert call(blobs, (1,), True, header_cap=-1)[0] == INVALID
    assert call([], (1,), True)[0] == INVALID
    assert call(blobs, (1,), True, device=99)[0] == NO_DEVICE
    assert call(blobs, (1,), True, device=-1)[0] == NO_DEVICE
    assert call(blobs, (1,), True)[0] == OK
    # bytes that are no UTF-8 are ordinary bytes: the call never fails on content
    st, headers, chunks, _, nh, nc = call([b"\xff\xfe\n# \xe2\x80\n\xc2", b"#\xc2"], (1,), True)
    assert st == OK and (nh, nc) == (1, 3) and headers[0].tolist() == [0, 1, 3, 7, 5, 7, 9, 0]
