"""Test helper: rules R1-R8 of the markdown chunker (include/vrag_amd.h) restated over UTF-8 bytes, one
line at a time.  `tables` returns the header and chunk records `vrag_chunk_markdown` must produce for one document,
`structural` the (raw, enhanced, header-path titles) chunks, `chunk_ref` the reference's list of (raw, enhanced) tuples.
tests/test_chunker_host.py pins all three to what the reference's own chunker returned (tests/golden/chunker_fixtures.json)."""
import re

_WS = rb"(?:[\x09-\x0d\x1c-\x20]|\xc2[\x85\xa0]|\xe1\x9a\x80|\xe2\x80[\x80-\x8a\xa8\xa9\xaf]|\xe2\x81\x9f|\xe3\x80\x80)"
_SPACE = re.compile(_WS)               # one character of Python's str.isspace set
_SPACES = re.compile(_WS + rb"*")
_TRAILING = re.compile(_WS + rb"+\Z")


def encode(text: str) -> bytes:
    return text.encode("utf-8", "surrogatepass")


def decode(data: bytes) -> str:
    return data.decode("utf-8", "surrogatepass")


def tables(data: bytes, split_levels=(1, 2, 3, 4), include_preamble=True, doc=0, header_base=0):
    """(headers, chunks): rows of 8 and 10 ints in the field order of vrag_md_header / vrag_md_chunk; header indexes start at
    `header_base`."""
    n = len(data)
    headers, last_e, s = [], -1, 0
    while s < n:                                                    # R1
        nl = data.find(b"\n", s)
        line_end = n if nl < 0 else nl
        k = 0
        while k < 7 and s + k < n and data[s + k] == 0x23:
            k += 1
        if 1 <= k <= 6 and _SPACE.match(data, s + k) and s > last_e:   # R2, R4
            p = _SPACES.match(data, s + k).end()                   # R3
            e = data.find(b"\n", p)
            e = n if e < 0 else e
            trail = _TRAILING.search(data, p, e)
            headers.append([doc, k, s, line_end, p, trail.start() if trail else e, n, 0])
            last_e = e
        if nl < 0:
            break
        s = nl + 1
    for a, b in zip(headers, headers[1:]):
        a[6] = b[2]                                                 # R7: a block ends where the next header's line starts
    if not headers:
        return [], [[doc, 0, n, -1, 0, -1, -1, -1, -1, -1]]          # R5
    chunks = []
    if include_preamble and headers[0][2] > 0:                      # R6
        chunks.append([doc, 0, headers[0][2], -1, 0, -1, -1, -1, -1, -1])
    stack = []
    for i, h in enumerate(headers):
        while stack and headers[stack[-1]][1] >= h[1]:
            stack.pop()
        if h[1] in split_levels:                                    # R8
            anc = [header_base + j for j in stack]
            chunks.append([doc, h[2], h[6], header_base + i, len(anc)] + anc + [-1] * (5 - len(anc)))
        stack.append(i)
    return headers, chunks


def structural(text: str, split_levels=(1, 2, 3, 4), include_preamble=True):
    """[(raw, enhanced, path)]: path = the titles of the ancestors and of the chunk's own header."""
    data = encode(text)
    headers, chunks = tables(data, split_levels, include_preamble)
    out = []
    for c in chunks:
        raw = decode(data[c[1]:c[2]])
        if c[3] < 0:
            out.append((raw, raw, ["Preamble" if headers else "Document"]))
            continue
        anc = [headers[j] for j in c[5:5 + c[4]]]
        lines = [decode(data[h[2]:h[3]]) for h in anc]
        out.append((raw, "\n".join(lines) + "\n\n" + raw if lines else raw, [decode(data[h[4]:h[5]]) for h in anc + [headers[c[3]]]]))
    return out


def chunk_ref(text: str, split_levels=(1, 2, 3, 4), include_preamble=True):
    return [(raw, enhanced) for raw, enhanced, _ in structural(text, split_levels, include_preamble)]
