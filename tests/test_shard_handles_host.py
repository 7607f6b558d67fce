"""Ownership of library handles in verbatim_rag_amd/shards.py (`_Handle` and its four wrappers) and the search-output helper,
against a stand-in for `_lib.load()` that records every call: no library, no device."""
import ctypes as C
import gc
import sys

import numpy as np
import pytest

import verbatim_rag_amd  # noqa: F401
from verbatim_rag_amd import _lib, shards


class FakeLib:
    """Every attribute is a library function that records (name, args) and returns status 0 (-1 for the names in `fail`); a
    `*_create` call hands out the next handle value through its last argument."""

    def __init__(self, fail=()):
        self.calls, self.fail, self.handles = [], set(fail), 0

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            if name in self.fail:
                return -1
            if name.endswith("_create"):
                self.handles += 1
                args[-1]._obj.value = 0x1000 * self.handles
            return 0
        return fn

    def destroyed(self):
        return [(name, args[0].value) for name, args in self.calls if name.endswith("_destroy")]


@pytest.fixture()
def lib(monkeypatch):
    fake = FakeLib()
    monkeypatch.setattr(_lib, "load", lambda: fake)
    monkeypatch.setattr(_lib, "require_gpu", lambda: None)
    return fake


def _make(kind):
    csr = (np.zeros(3, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32))
    if kind == "ivf":
        return shards.IvfOverlay(shards.DenseShard(4, 8), 2)
    return {"dense": lambda: shards.DenseShard(4, 8), "sparse": lambda: shards.SparseShard(10, *csr),
            "text": lambda: shards.TextIndex()}[kind]()


DESTROY = {"dense": "vrag_dense_index_destroy", "ivf": "vrag_ivf_index_destroy", "sparse": "vrag_sparse_index_destroy",
           "text": "vrag_text_index_destroy"}


@pytest.mark.parametrize("kind", ["dense", "ivf", "sparse", "text"])
def test_close_destroys_once(lib, kind):
    obj = _make(kind)
    handle = obj._h.value
    assert handle and isinstance(obj, shards._Handle) and (DESTROY[kind], handle) not in lib.destroyed()
    obj.close()
    assert (DESTROY[kind], handle) in lib.destroyed() and not obj._h
    n = len(lib.calls)
    obj.close()
    del obj
    gc.collect()
    assert len(lib.calls) == n                                  # neither a second close nor the collector calls anything
    assert len(lib.destroyed()) == len({h for _name, h in lib.destroyed()}) == lib.handles      # every handle, each once


@pytest.mark.parametrize("kind", ["dense", "ivf", "sparse", "text"])
def test_a_failed_constructor_is_collected_quietly(lib, monkeypatch, kind):
    raised = []
    monkeypatch.setattr(sys, "unraisablehook", lambda info: raised.append(info))
    lib.fail.add(DESTROY[kind].replace("_destroy", "_create"))
    cls = {"dense": shards.DenseShard, "ivf": shards.IvfOverlay, "sparse": shards.SparseShard, "text": shards.TextIndex}[kind]
    with pytest.raises(_lib.VragError):
        _make(kind)                                             # raises inside `_lib.check`, after `_h` exists (null)
    bare = cls.__new__(cls)                                     # a constructor that failed before `_h` was assigned
    bare.close()
    del bare
    gc.collect()
    assert not raised
    assert DESTROY[kind] not in [name for name, _h in lib.destroyed()]      # no handle was made: nothing of this kind to destroy


def test_dense_shard_closes_its_overlay_first(lib):
    shard = shards.DenseShard(4, 8)
    shard.ivf = shards.IvfOverlay(shard, 2)
    h_shard, h_ivf = shard._h.value, shard.ivf._h.value
    shard.close()
    assert lib.destroyed() == [("vrag_ivf_index_destroy", h_ivf), ("vrag_dense_index_destroy", h_shard)]
    assert shard.ivf is None
    shard.close()
    assert len(lib.destroyed()) == 2


@pytest.mark.parametrize("nq,k", [(0, 5), (1, 1), (3, 65)])
def test_output_helper(nq, k):
    for fill in (False, True):
        scores, ids, sp, ip = shards._topk_out(nq, k, fill=fill)
        assert scores.shape == ids.shape == (nq, k) and scores.dtype == np.float32 and ids.dtype == np.int64
        assert scores.flags.c_contiguous and ids.flags.c_contiguous
        assert isinstance(sp, shards._FP) and isinstance(ip, shards._LP)
        if nq:
            assert C.addressof(sp.contents) == scores.ctypes.data and C.addressof(ip.contents) == ids.ctypes.data
        if fill:
            assert (scores == -np.inf).all() and (ids == -1).all()
