#!/usr/bin/env python3
"""Markdown chunker probe -> profiles/chunker_probe.txt.

  python tools/probes/chunker_probe.py [--out FILE]                 on the GPU machine: the timings
  python tools/probes/chunker_probe.py --host-part <reference>      where a reference checkout is: the reference chunker's own
                                                                    time on the same corpora (three runs) and the kernels' registers, into
                                                                    profiles/chunker_probe_host_part.txt, which the first form
                                                                    quotes as taken on another host

Timings: host clock around synchronous calls, one warm-up call, then the median of 5 (min and max beside it).  Per corpus: the
device call alone (`vrag_chunk_markdown` on prepared buffers), GpuMarkdownChunker.chunk_batch (encode + device call + string
building), and tests/chunk_ref.py -- the line-by-line Python restatement of the same rules -- on the same host, timed once.
Corpora come from a seed: 250 documents of about 8 KB built by tests/golden/gen_golden_chunker.synth_markdown, repeated / joined
to the sizes below."""
import argparse
import ctypes as C
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]
HOST_PART = os.path.join(ROOT, "profiles", "chunker_probe_host_part.txt")


def corpora(which=None):
    from gen_golden_chunker import synth_markdown

    pool = [synth_markdown(random.Random(31000 + i), 8192) for i in range(250)]
    rng = random.Random(5)
    out = {}
    if which in (None, "10k x 8 KB"):
        out["10k x 8 KB"] = [pool[i % 250] for i in range(10_000)]
    if which in (None, "100 x 1 MB"):
        out["100 x 1 MB"] = ["".join(rng.choice(pool) for _ in range(128)) for _ in range(100)]
    if which in (None, "1 x 64 MB"):
        out["1 x 64 MB"] = ["".join(pool[i % 250] for i in range(8192))]
    if which in (None, "adversarial"):
        out["adversarial"] = ["# " + "x" * (16 << 20)]       # one title line of 16 MB: one lane walks it alone
    return out


def timed(fn, reps=5):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def device_part(out_path):
    import numpy as np

    import chunk_ref
    from verbatim_rag_amd import _lib
    from verbatim_rag_amd.chunker_providers import GpuMarkdownChunker

    lib = _lib.load()
    _lib.require_gpu()
    lines = ["markdown chunker probe: ms, host clock around synchronous calls, one warm-up then median of 5 (min, max), one process",
             "default settings: split_levels (1, 2, 3, 4), preamble, no size limits; chunk_ref (Python, same host) timed once", "",
             f"{'corpus':>12} {'MB':>7} {'headers':>8} {'chunks':>8}  {'device call':>24}  {'chunk_batch (strings)':>24}  {'chunk_ref':>10}"]
    chunker = GpuMarkdownChunker()
    for name, texts in corpora().items():
        blobs = [t.encode("utf-8") for t in texts]
        off = np.zeros(len(blobs) + 1, np.int64)
        np.cumsum([len(b) for b in blobs], out=off[1:])
        hcap = sum(b.count(b"\n#") + 1 for b in blobs)
        headers, chunks = np.empty((hcap, 8), np.int32), np.empty((hcap + len(blobs), 10), np.int32)
        dco = np.empty(len(blobs) + 1, np.int64)
        nh, nc = C.c_int64(0), C.c_int64(0)
        blob = b"".join(blobs)
        buf = (C.c_char * len(blob)).from_buffer_copy(blob)

        def device_call():
            _lib.check("vrag_chunk_markdown", lib.vrag_chunk_markdown(
                C.cast(buf, C.c_void_p), off.ctypes.data_as(C.POINTER(C.c_int64)), len(blobs), 0b11110, 1, hcap,
                headers.ctypes.data_as(C.c_void_p), hcap + len(blobs), chunks.ctypes.data_as(C.c_void_p), C.byref(nh), C.byref(nc),
                dco.ctypes.data_as(C.POINTER(C.c_int64)), 0))

        dev = timed(device_call)
        full = timed(lambda: chunker.chunk_batch(texts))
        t = time.perf_counter()
        want = [chunk_ref.chunk_ref(x) for x in texts]
        ref_ms = (time.perf_counter() - t) * 1e3
        assert chunker.chunk_batch(texts) == want, name
        fmt = lambda m: f"{m[0]:9.2f} ({m[1]:.2f}, {m[2]:.2f})"
        lines.append(f"{name:>12} {len(blob) / 1e6:7.1f} {nh.value:8d} {nc.value:8d}  {fmt(dev):>24}  {fmt(full):>24}  {ref_ms:10.0f}")
        print(lines[-1], flush=True)
    lines += ["", "the adversarial document is '# ' and one 16 MB line: the candidate's own lane walks the title to its end, 16 bytes per load, so",
              "the call takes as long as one lane needs to read 16 MB (DESIGN.md section 3); the bytes of every other corpus are spread over",
              "the chip 16 bytes per lane.  1 x 64 MB: one lane walks the document's 464 069 headers alone (twice), most of that call.", ""]
    if os.path.exists(HOST_PART):
        with open(HOST_PART) as f:
            lines += ["taken on ANOTHER host (a CPU-only machine, not this one's host):"] + ["  " + l.rstrip("\n") for l in f]
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


def host_part(ref):
    sys.path.insert(0, os.path.abspath(ref))
    import importlib.util

    spec = importlib.util.spec_from_file_location("_ref_chunkers", os.path.join(ref, "verbatim_rag", "chunker_providers.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lines = ["reference MarkdownChunkerProvider().chunk per document, default settings, three runs (min .. max):"]
    for name, take in (("10k x 8 KB", 10_000), ("100 x 1 MB", 2)):
        texts = corpora(name)[name][:take]
        ms = []
        for _ in range(3):
            t = time.perf_counter()
            n = sum(len(mod.MarkdownChunkerProvider().chunk(x)) for x in texts)
            ms.append((time.perf_counter() - t) * 1e3)
        lines.append(f"  {name:>12}: {take} documents, {n} chunks, {min(ms):.0f} .. {max(ms):.0f} ms"
                     + (f" = {min(ms) / take:.0f} .. {max(ms) / take:.0f} ms per document" if take < 100 else ""))
        print(lines[-1], flush=True)
    lines.append("  (1 x 64 MB is not run: its header-to-line walk grows with headers x lines)")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"),
                          os.path.join(ROOT, "verbatim-rag_amd", "csrc", "chunk.hip")], capture_output=True, text=True, check=True).stdout
    lines += ["tools/kernel_resources.py verbatim-rag_amd/csrc/chunk.hip:"] + ["  " + l[:110] for l in res.splitlines()]
    with open(HOST_PART, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chunker_probe.txt"))
    ap.add_argument("--host-part", metavar="REFERENCE")
    a = ap.parse_args()
    host_part(a.host_part) if a.host_part else device_part(a.out)
