"""On-disk format helpers of `GpuVectorStore.save` / `.load`: atomic file replacement, string columns, and the reader of
every saved format."""
from __future__ import annotations

import json
from typing import Any, Dict, List, Sequence

import numpy as np

_NO_METADATA: Dict[str, Any] = {}


def _replace_into(path: str, name: str, writer) -> None:
    """Writes beside the final name and renames into place: a reader never sees half a file."""
    import os

    tmp = os.path.join(path, f".{name}.tmp{os.getpid()}")
    writer(tmp)
    os.replace(tmp, os.path.join(path, name))


def _write_text(file: str, text: str) -> None:
    with open(file, "w", encoding="utf-8", newline="") as f:
        f.write(text)


def _put_strings(path: str, stem: str, col: Sequence[str]) -> None:
    """A column of strings as `{stem}.txt`: the rows joined by NUL (one C-level join / split for 10^7 rows); a column
    holding a NUL itself or a non-string goes to `{stem}.json` instead."""
    import os

    blob = None
    try:
        blob = "\x00".join(col)
        if blob.count("\x00") != max(0, len(col) - 1):
            blob = None
    except TypeError:
        blob = None
    # new file first (write beside + rename: a reader never sees the column missing), then the other extension's stale file
    if blob is not None:
        _replace_into(path, f"{stem}.txt", lambda tmp: _write_text(tmp, blob))
        stale = f"{stem}.json"
    else:
        _replace_into(path, f"{stem}.json", lambda tmp: _write_text(tmp, json.dumps(list(col), ensure_ascii=False)))
        stale = f"{stem}.txt"
    if os.path.exists(os.path.join(path, stale)):
        os.remove(os.path.join(path, stale))


def _get_strings(path: str, stem: str, n: int) -> List[str]:
    import os

    txt, js = os.path.join(path, f"{stem}.txt"), os.path.join(path, f"{stem}.json")

    def read_txt():
        with open(txt, encoding="utf-8", newline="") as f:
            return f.read().split("\x00") if n else []

    def read_json():
        with open(js, encoding="utf-8") as f:
            return json.load(f)

    if os.path.exists(txt) and os.path.exists(js):
        # an overwrite was interrupted between the rename of the new file and the removal of the old one: the newer file wins;
        # with equal timestamps (coarse clocks, restored backups) the one that holds the manifest's row count does
        mt, mj = os.path.getmtime(txt), os.path.getmtime(js)
        if mt != mj:
            col = read_json() if mj > mt else read_txt()
        else:
            col = read_txt()
            if len(col) != n:
                col = read_json()
    elif os.path.exists(txt):
        col = read_txt()
    else:
        col = read_json()
    if len(col) != n:
        raise ValueError(f"{path}: {stem} holds {len(col)} rows, expected {n}")
    return col


def put_pq_codebooks(arrays: Dict[str, np.ndarray], codebooks, trained_rows: int) -> None:
    """The frozen codebooks of an index_type="PQ" store as one more array of the rank's `vectors.rank{r}.npz` (and the size of
    the sample they were trained on); a store that has not trained yet writes neither."""
    if codebooks is not None:
        arrays["pq_codebooks"] = np.ascontiguousarray(codebooks, dtype=np.float32)
        arrays["pq_trained_rows"] = np.asarray([int(trained_rows)], dtype=np.int64)


def get_pq_codebooks(arrays, m: int, dense_dim: int):
    """(codebooks float32 `[m, 256, dense_dim // m]` or None, trained rows) from the arrays `put_pq_codebooks` wrote into."""
    if "pq_codebooks" not in arrays:
        return None, 0
    cb = np.ascontiguousarray(arrays["pq_codebooks"], dtype=np.float32)
    if cb.shape != (m, 256, dense_dim // m):
        raise ValueError(f"saved PQ codebooks have shape {cb.shape}, expected {(m, 256, dense_dim // m)}")
    return cb, int(np.asarray(arrays["pq_trained_rows"]).reshape(-1)[0]) if "pq_trained_rows" in arrays else 0


def read_saved(path: str):
    """Any on-disk format -> (head, ids, [per saved rank: (owned rows, arrays, texts, enhanced, metadatas)]).
    Format 3 = `GpuVectorStore.save`; format 2 = `rows.json` holding ids / texts / metadata for all rows beside
    `vectors.rank{r}.npz`; format 1 = `rows.json` + one `vectors.npz` in row order (single GPU)."""
    import os

    def get_json(name):
        with open(os.path.join(path, name), encoding="utf-8") as f:
            return json.load(f)

    if os.path.exists(os.path.join(path, "store.json")):
        head = get_json("store.json")
        if head.get("format") != 3:
            raise ValueError(f"{path}: unknown GpuVectorStore format {head.get('format')!r}")
        ids = _get_strings(path, "ids", head["rows"])
        shards = []
        for r in range(head.get("world", 1)):
            z = np.load(os.path.join(path, f"vectors.rank{r}.npz"))
            m = len(z["owned"])
            metas = get_json(f"metadatas.rank{r}.json")
            if isinstance(metas, dict):
                metas = [_NO_METADATA] * int(metas["empty_rows"])
            if len(metas) != m:
                raise ValueError(f"{path}: metadatas.rank{r} holds {len(metas)} rows, expected {m}")
            shards.append((z["owned"], z, _get_strings(path, f"texts.rank{r}", m), _get_strings(path, f"enhanced.rank{r}", m), metas))
        return head, ids, shards
    rows = get_json("rows.json")
    fmt = rows.get("format")
    if fmt not in (1, 2):
        raise ValueError(f"{path}: unknown GpuVectorStore format {fmt!r}")
    ids = list(rows["ids"])
    head = {k: rows.get(k) for k in ("dense_dim", "sparse_vocab", "enable_dense", "enable_sparse", "dense_dtype")}
    head.update(world=rows.get("world", 1) if fmt == 2 else 1, rows=len(ids), documents=rows.get("documents", []))
    shards = []
    for r in range(head["world"]):
        z = np.load(os.path.join(path, "vectors.npz" if fmt == 1 else f"vectors.rank{r}.npz"))
        owned = np.arange(len(ids), dtype=np.int64) if fmt == 1 else z["owned"]
        shards.append((owned, z, [rows["texts"][g] for g in owned], [rows["enhanced_texts"][g] for g in owned],
                       [rows["metadatas"][g] for g in owned]))
    return head, ids, shards
