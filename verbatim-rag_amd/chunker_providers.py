"""Chunker providers: the reference's module of the same name (verbatim_rag/chunker_providers.py) with its default chunker,
MarkdownChunkerProvider, on the GPU.

The structural pass -- where the headers are, which block becomes a chunk, which headers are its ancestors -- is byte work
over the whole document and runs on the device for a batch of documents at once (`vrag_chunk_markdown`, csrc/chunk.hip; rules
R1-R8 in include/vrag_amd.h).  It returns two small record tables of byte offsets; the strings are slices of the document's
UTF-8 bytes at those offsets.  The optional size stages (merge chunks under `min_chunk_size`, split chunks over
`max_chunk_size` at paragraph breaks outside tables and code fences) act on chunks, not bytes, and stay on the host:
`apply_size_limits`, the reference's output quirk for quirk but without its every-break-against-every-region loops.

ChonkieChunkerProvider / SimpleChunkerProvider stay with the reference."""
from __future__ import annotations

import re
from abc import ABC, abstractmethod
from bisect import bisect_left, bisect_right
from typing import List, Optional, Sequence, Tuple

MAX_BATCH_BYTES = 512 << 20   # VRAG_MD_MAX_BATCH_BYTES

# (raw chunk, enhanced chunk, header path): the path holds the titles of the chunk's ancestors and of its own header
StructuralChunk = Tuple[str, str, List[str]]


class ChunkerProvider(ABC):
    """chunk(text) -> [(raw_chunk, enhanced_chunk)]: the raw text for extraction / display and the text with its structural
    context (ancestor headings) for embedding.  Document metadata is added by the index, not here."""

    @abstractmethod
    def chunk(self, text: str) -> List[Tuple[str, str]]:
        ...


# ---------------------------------------------------------------------------------------------------------------- size stages
_TABLE = re.compile(r"(?:^[ ]*\|.+\n)+", re.MULTILINE)                # contiguous lines that open with |
_TABLE_RULE = re.compile(r"\|[-:\s]+\|")                              # ... and hold a |---| row
_CAPTION = re.compile(r"^[ ]*Table\s+\d+[:\.].*$", re.MULTILINE)
_FENCE = re.compile(r"```[a-zA-Z0-9+\-_]*\n.*?\n```", re.DOTALL)
_PARAGRAPH_BREAK = re.compile(r"\n\n+")


def _join(a: StructuralChunk, b: StructuralChunk) -> StructuralChunk:
    """Two neighbours as one chunk.  The enhanced texts are concatenated as they are (the second one's ancestor prefix lands in
    the middle) and the first one's header path is kept."""
    return a[0] + b[0], a[1] + b[1], a[2]


def _merge_small(chunks: Sequence[StructuralChunk], min_size: int) -> List[StructuralChunk]:
    """A chunk shorter than min_size (characters of raw text) joins the chunk behind it, again and again while the result is
    still short; a short last chunk joins the result before it."""
    chunks = list(chunks)
    out: List[StructuralChunk] = []
    i, n = 0, len(chunks)
    while i < n:
        small = len(chunks[i][0]) < min_size
        if small and i + 1 < n:
            both = _join(chunks[i], chunks[i + 1])
            if len(both[0]) < min_size and i + 2 < n:
                chunks[i + 1] = both       # still short: it stands in for its second half and is looked at again
                i += 1
            else:
                out.append(both)
                i += 2
        elif small and out:                # the last chunk
            out[-1] = _join(out[-1], chunks[i])
            i += 1
        else:
            out.append(chunks[i])
            i += 1
    return out


class _Regions:
    """The protected regions of a document -- tables with their `Table N:` caption, code fences -- as half-open character
    spans, sorted by start, with the running maximum of their ends: `covers(pos)` is one bisection whatever the number of regions
    (they may overlap)."""

    def __init__(self, text: str):
        tables = [(m.start(), m.end()) for m in _TABLE.finditer(text) if _TABLE_RULE.search(m.group())]
        table_starts = [a for a, _ in tables]
        captions = [(m.start(), m.end()) for m in _CAPTION.finditer(text)]
        cap_starts = [a for a, _ in captions]
        cap_ends = [z for _, z in captions]
        spans = []
        for a, z in tables:
            lo, hi = a, z
            # a caption in front: only the nearest one can have nothing but white space between itself and the table
            j = bisect_right(cap_ends, a) - 1
            if j >= 0 and text[cap_ends[j]:a].strip() == "" \
                    and bisect_left(table_starts, a) <= bisect_right(table_starts, cap_ends[j]):   # no table starts in between
                lo = cap_starts[j]
            # a caption behind: the first one, unless some table starts behind that caption (then it is that table's)
            j = bisect_left(cap_starts, z)
            if j < len(captions) and text[z:cap_starts[j]].strip() == "" and not (table_starts and table_starts[-1] > cap_ends[j]):
                hi = cap_ends[j]
            spans.append((lo, hi))
        spans += [(m.start(), m.end()) for m in _FENCE.finditer(text)]
        spans.sort()
        self.starts = [a for a, _ in spans]
        self.reach: List[int] = []          # reach[i] = the largest end among spans[0..i]
        for _, z in spans:
            self.reach.append(max(z, self.reach[-1]) if self.reach else z)

    def covers(self, pos: int) -> bool:
        i = bisect_right(self.starts, pos) - 1
        return i >= 0 and self.reach[i] > pos


def _split_points(raw: str, offset: int, regions: _Regions) -> List[int]:
    """Starts of the paragraph breaks of `raw` (at `offset` in the document) that do not lie in protected text at both ends.  (The
    reference also asks that no single region holds the whole break; a break inside one region has both ends covered, so that is
    the same condition.)"""
    return [m.start() for m in _PARAGRAPH_BREAK.finditer(raw)
            if not (regions.covers(offset + m.start()) and regions.covers(offset + m.end() - 1))]


def _split_large(chunks: Sequence[StructuralChunk], document: str, max_size: int) -> List[StructuralChunk]:
    regions: Optional[_Regions] = None
    out: List[StructuralChunk] = []
    for chunk in chunks:
        raw, _, path = chunk
        if len(raw) <= max_size:
            out.append(chunk)
            continue
        if regions is None:
            regions = _Regions(document)
        # the chunk is placed at the FIRST occurrence of its text; a merged chunk that spans a dropped block occurs nowhere and
        # is placed at -1, as the reference places it
        points = _split_points(raw, document.find(raw), regions)
        if not points:
            out.append(chunk)
            continue
        # sub-chunks name their ancestors as `## title` lines whatever the levels were
        prefix = "\n".join(f"## {t}" for t in path[:-1]) + "\n\n" if len(path) > 1 else ""
        current = ""
        prev = 0
        for pos in points + [len(raw)]:     # ascending and distinct already
            part = raw[prev:pos]
            prev = pos
            if not part.strip():
                continue
            if current and len(current) + len(part) > max_size:
                out.append((current, prefix + current, path))
                current = part
            else:
                current += part
        if current:
            out.append((current, prefix + current, path))
    return out


def apply_size_limits(chunks: Sequence[StructuralChunk], document: str, min_chunk_size: Optional[int] = None,
                      max_chunk_size: Optional[int] = None) -> List[Tuple[str, str]]:
    """The reference's size stages over the structural chunks of `document` (chunker_providers.py:284-455): merge the tiny
    ones, split the large ones at paragraph breaks outside tables and code fences, merge again what the split left tiny (only
    when a minimum is set).  Sizes are characters of raw text."""
    chunks = list(chunks)
    if min_chunk_size is not None:
        chunks = _merge_small(chunks, min_chunk_size)
    if max_chunk_size is not None:
        chunks = _split_large(chunks, document, max_chunk_size)
        if min_chunk_size is not None:
            chunks = _merge_small(chunks, min_chunk_size)
    return [(raw, enhanced) for raw, enhanced, _ in chunks]


# ---------------------------------------------------------------------------------------------------------------- the chunker
def _levels_mask(split_levels) -> int:
    mask = 0
    for level in split_levels:
        if isinstance(level, int) and 1 <= level <= 6:   # other values can never equal a header's level
            mask |= 1 << level
    return mask


class GpuMarkdownChunker(ChunkerProvider):
    """MarkdownChunkerProvider (chunker_providers.py:35-455) with the structural pass on the GPU.  `chunk_batch` takes many
    documents through one device call (cut at 512 MiB of text); no device, no result: there is no CPU fallback."""

    def __init__(self, split_levels: tuple = (1, 2, 3, 4), include_preamble: bool = True, min_chunk_size: Optional[int] = None,
                 max_chunk_size: Optional[int] = None, device: int = 0):
        self.split_levels = split_levels
        self.include_preamble = include_preamble
        self.min_chunk_size = min_chunk_size
        self.max_chunk_size = max_chunk_size
        self.device = device

    def chunk(self, text: str) -> List[Tuple[str, str]]:
        return self.chunk_batch([text])[0]

    def chunk_batch(self, texts: Sequence[str]) -> List[List[Tuple[str, str]]]:
        texts = list(texts)
        # lone surrogates survive the round trip, so such a str chunks like any other
        blobs = [t.encode("utf-8", "surrogatepass") for t in texts]
        sized = self.min_chunk_size is not None or self.max_chunk_size is not None
        out: List[List[Tuple[str, str]]] = []
        a = 0
        while a < len(blobs):
            b, total = a + 1, len(blobs[a])
            while b < len(blobs) and total + len(blobs[b]) <= MAX_BATCH_BYTES:
                total += len(blobs[b])
                b += 1
            for text, chunks in zip(texts[a:b], self._structural(blobs[a:b], with_paths=sized)):
                if sized:
                    out.append(apply_size_limits(chunks, text, self.min_chunk_size, self.max_chunk_size))
                else:
                    out.append([(raw, enhanced) for raw, enhanced, _ in chunks])
            a = b
        return out

    def records(self, blobs: Sequence[bytes]):
        """The two record tables of one device call over `blobs` (UTF-8 documents): (headers [n, 8], chunks [n, 10], doc_chunk_off
        [len(blobs) + 1]) as int32 / int32 / int64 arrays in the field order of vrag_md_header / vrag_md_chunk."""
        import ctypes as C

        import numpy as np

        from . import _lib

        lib = _lib.load()
        _lib.require_gpu()
        off = np.zeros(len(blobs) + 1, np.int64)
        np.cumsum([len(b) for b in blobs], out=off[1:])
        # a header needs a line that begins with '#': one per "\n#", and the first line
        header_cap = sum(b.count(b"\n#") + 1 for b in blobs)
        chunk_cap = header_cap + len(blobs)
        headers = np.empty((header_cap, 8), np.int32)
        chunks = np.empty((chunk_cap, 10), np.int32)
        doc_chunk_off = np.empty(len(blobs) + 1, np.int64)
        n_headers, n_chunks = C.c_int64(0), C.c_int64(0)
        blob = b"".join(blobs) or b"\x00"
        buf = (C.c_char * len(blob)).from_buffer_copy(blob)
        _lib.check("vrag_chunk_markdown", lib.vrag_chunk_markdown(
            C.cast(buf, C.c_void_p), off.ctypes.data_as(C.POINTER(C.c_int64)), len(blobs), _levels_mask(self.split_levels),
            1 if self.include_preamble else 0, header_cap, headers.ctypes.data_as(C.c_void_p), chunk_cap,
            chunks.ctypes.data_as(C.c_void_p), C.byref(n_headers), C.byref(n_chunks),
            doc_chunk_off.ctypes.data_as(C.POINTER(C.c_int64)), self.device))
        return headers[: n_headers.value], chunks[: n_chunks.value], doc_chunk_off

    def _structural(self, blobs: Sequence[bytes], with_paths: bool) -> List[List[StructuralChunk]]:
        headers, chunks, doc_chunk_off = self.records(blobs)
        headers, chunks, bounds = headers.tolist(), chunks.tolist(), doc_chunk_off.tolist()
        out: List[List[StructuralChunk]] = []
        for d, data in enumerate(blobs):
            rows = chunks[bounds[d]:bounds[d + 1]]
            doc: List[StructuralChunk] = []
            for _, start, end, header, n_anc, *anc in rows:
                raw = data[start:end].decode("utf-8", "surrogatepass")
                if header < 0:              # the preamble, or a document without headers
                    doc.append((raw, raw, ["Document"]))   # a path of one: no ancestors
                    continue
                above = [headers[j] for j in anc[:n_anc]]
                enhanced = raw
                if above:
                    enhanced = "\n".join(data[h[2]:h[3]].decode("utf-8", "surrogatepass") for h in above) + "\n\n" + raw
                path = [data[h[4]:h[5]].decode("utf-8", "surrogatepass") for h in above + [headers[header]]] if with_paths else []
                doc.append((raw, enhanced, path))
            out.append(doc)
        return out
