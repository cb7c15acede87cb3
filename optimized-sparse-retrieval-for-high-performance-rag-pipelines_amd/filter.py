"""Doc filters (include/sparse_rx_filter.h): restrict a sparse or a dense search to a set of docs.

A filter row is a bitmap over the shard-local rows of an index -- doc ``d`` is allowed iff bit ``d & 31`` of word
``d >> 5`` is set --, :func:`filter_words` 32-bit words long; a :class:`DocFilter` is ``n_filters`` such rows in one device
tensor.  A search takes the filter and, optionally, ``q_filter`` i32[nq]: the row of every query (``None``: row 0 for
all; ``-1``: that query is not filtered).  The reference has no filters: nothing here mirrors reference code.
"""
from __future__ import annotations

import ctypes
from typing import Sequence

import numpy as np

from . import _capi


def _torch():
    import torch
    return torch


def filter_words(n_docs: int) -> int:
    """``srx_filter_words``: words per row -- ceil(n_docs / 32) rounded up to a multiple of 4 (rows stay 16-byte aligned)."""
    if not (1 <= int(n_docs) <= 2 ** 31 - 2):
        raise ValueError(f"n_docs must be in [1, 2^31 - 2], got {n_docs}")
    return ((int(n_docs) + 31) // 32 + 3) // 4 * 4


def pack_masks(masks) -> np.ndarray:
    """bool[n_docs] or bool[n_filters, n_docs] -> uint32[n_filters, filter_words(n_docs)] (tail bits and padding words 0)."""
    m = np.asarray(masks)
    if m.dtype != np.bool_:
        raise ValueError("a filter mask must be a bool array")
    if m.ndim == 1:
        m = m[None, :]
    if m.ndim != 2 or m.shape[0] < 1 or m.shape[1] < 1:
        raise ValueError("a filter mask must be bool[n_docs] or bool[n_filters, n_docs] with n_filters, n_docs >= 1")
    words = filter_words(m.shape[1])
    out = np.zeros((m.shape[0], words * 4), dtype=np.uint8)
    packed = np.packbits(m, axis=1, bitorder="little")
    out[:, : packed.shape[1]] = packed
    return out.view("<u4")


def validate_q_filter(q_filter, nq: int, n_filters: int):
    """The host-array door's check of ``q_filter``: None, or nq integers in [-1, n_filters).  Returns int32[nq] or None."""
    if q_filter is None:
        return None
    q = np.asarray(q_filter)
    if q.ndim != 1 or q.shape[0] != nq or not np.issubdtype(q.dtype, np.integer):
        raise ValueError(f"q_filter must be {nq} integers (one filter row per query)")
    if q.size and (int(q.min()) < -1 or int(q.max()) >= n_filters):
        raise ValueError(f"q_filter values must lie in [-1, {n_filters}): -1 = not filtered, else a row of the filter")
    return np.ascontiguousarray(q, dtype=np.int32)


class DocFilter:
    """``n_filters`` filter rows over the ``n_docs`` local rows of one index (sparse, dense f32 or dense uint8) whose first
    row has the GLOBAL id ``doc_base``.  ``bits`` is an int32 tensor [n_filters, filter_words(n_docs)] on ``device``."""

    def __init__(self, bits, n_docs: int, doc_base: int = 0):
        torch = _torch()
        words = filter_words(n_docs)
        if bits.dtype != torch.int32 or bits.dim() != 2 or int(bits.shape[1]) != words or int(bits.shape[0]) < 1 or not bits.is_contiguous():
            raise ValueError(f"filter bits must be a contiguous int32 tensor [n_filters >= 1, {words}]")
        if bits.data_ptr() % 16:
            raise ValueError("filter bits must be 16-byte aligned")
        self.bits, self.n_docs, self.doc_base, self.device = bits, int(n_docs), int(doc_base), bits.device
        self.n_filters, self.words = int(bits.shape[0]), words

    # -- constructors -----------------------------------------------------------------------------------------------
    @classmethod
    def from_masks(cls, masks, device="cuda:0", doc_base: int = 0) -> "DocFilter":
        """bool[n_docs] | bool[n_filters, n_docs] (True = allowed), packed on the host (:func:`pack_masks`) and uploaded."""
        torch = _torch()
        packed = pack_masks(masks)
        n_docs = np.asarray(masks).shape[-1]
        return cls(torch.from_numpy(packed.view(np.int32).copy()).to(torch.device(device)), n_docs, doc_base)

    @classmethod
    def filled(cls, n_filters: int, n_docs: int, value: bool, device="cuda:0", doc_base: int = 0) -> "DocFilter":
        """``srx_filter_fill``: every doc of every row allowed (True) or not (False)."""
        torch = _torch()
        dev = torch.device(device)
        if n_filters < 1:
            raise ValueError("a filter needs n_filters >= 1 rows")
        f = cls(torch.empty((int(n_filters), filter_words(n_docs)), dtype=torch.int32, device=dev), n_docs, doc_base)
        with torch.cuda.device(dev):
            rc = _capi.lib().srx_filter_fill(dev.index or 0, f.bits.data_ptr(), f.n_filters, f.n_docs, int(bool(value)),
                                            torch.cuda.current_stream(dev).cuda_stream)
        _capi.check(rc, "srx_filter_fill")
        return f

    @classmethod
    def allow(cls, id_lists, n_docs: int, device="cuda:0", doc_base: int = 0) -> "DocFilter":
        """One row per list of GLOBAL ids: only the listed docs are allowed (fill 0 + ``srx_filter_set_docs``)."""
        return cls._from_lists(id_lists, n_docs, device, doc_base, listed=True)

    @classmethod
    def deny(cls, id_lists, n_docs: int, device="cuda:0", doc_base: int = 0) -> "DocFilter":
        """One row per list of GLOBAL ids: every doc but the listed ones is allowed (fill 1 + ``srx_filter_set_docs``)."""
        return cls._from_lists(id_lists, n_docs, device, doc_base, listed=False)

    @classmethod
    def _from_lists(cls, id_lists, n_docs, device, doc_base, listed: bool) -> "DocFilter":
        lists = list(id_lists)
        if lists and np.ndim(lists[0]) == 0:
            lists = [lists]  # one list of ids = one row
        f = cls.filled(max(len(lists), 1), n_docs, not listed, device, doc_base)
        for r, ids in enumerate(lists):
            f.set_docs(r, ids, listed)
        return f

    # -- methods ----------------------------------------------------------------------------------------------------
    def set_docs(self, row: int, ids, value: bool) -> None:
        """``srx_filter_set_docs``: allow (True) or disallow (False) the listed GLOBAL ids in row ``row``, in place --
        tombstoning.  ``ids``: a host sequence or an int32 device tensor of any shape (a result block of a search can be
        passed as it is); ids outside this index, -1 included, are ignored; duplicates are legal.  Asynchronous."""
        torch = _torch()
        if not (0 <= int(row) < self.n_filters):
            raise ValueError(f"filter row {row} outside [0, {self.n_filters})")
        if isinstance(ids, torch.Tensor):
            if ids.dtype != torch.int32:
                raise ValueError("doc ids on the device must be an int32 tensor")
            t = ids.to(self.device).contiguous().reshape(-1)
        else:
            a = np.asarray(ids, dtype=np.int64).reshape(-1)
            if a.size and (int(a.min()) < -(2 ** 31) or int(a.max()) >= 2 ** 31):
                raise ValueError("doc ids must fit int32")
            t = torch.as_tensor(a.astype(np.int32), device=self.device)
        if t.numel() == 0:
            return
        with torch.cuda.device(self.device):
            rc = _capi.lib().srx_filter_set_docs(self.device.index or 0, self.bits[int(row)].data_ptr(), self.n_docs, self.doc_base,
                                                t.data_ptr(), t.numel(), int(bool(value)), torch.cuda.current_stream(self.device).cuda_stream)
        _capi.check(rc, "srx_filter_set_docs")

    def count(self) -> np.ndarray:
        """``srx_filter_count``: allowed docs per row, int32[n_filters] on the host (synchronises)."""
        torch = _torch()
        out = torch.empty((self.n_filters,), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            rc = _capi.lib().srx_filter_count(self.device.index or 0, self.bits.data_ptr(), self.n_filters, self.n_docs, out.data_ptr(),
                                             torch.cuda.current_stream(self.device).cuda_stream)
        _capi.check(rc, "srx_filter_count")
        return out.cpu().numpy()

    def for_index(self, ix) -> "DocFilter":
        """This filter, checked against the index it is about to restrict (``n_docs``, ``doc_base``, device).  Raises ValueError."""
        torch = _torch()
        if self.n_docs != int(ix.n_docs) or self.doc_base != int(ix.doc_base):
            raise ValueError(f"the filter speaks of {self.n_docs} docs from id {self.doc_base}, the index of {ix.n_docs} from {ix.doc_base}")
        if torch.device(ix.device) != self.device:
            raise ValueError(f"the filter lives on {self.device}, the index on {ix.device}")
        return self

    def launch_args(self, q_filter, nq: int):
        """The ``srx_doc_filter`` struct of one call and what must stay alive while the call is issued.  ``q_filter``: None or an
        int32 tensor [nq] on the filter's device (values in [-1, n_filters): NOT checked here, the tensor never leaves the
        device -- the host-array doors check theirs)."""
        torch = _torch()
        if q_filter is not None:
            if q_filter.dtype != torch.int32 or q_filter.numel() != nq or q_filter.device != self.device:
                raise ValueError(f"q_filter must be an int32 tensor [{nq}] on {self.device}")
            q_filter = q_filter.contiguous()
        desc = _capi.DocFilterDesc(bits=self.bits.data_ptr(), n_filters=self.n_filters,
                                   q_filter=None if q_filter is None or nq == 0 else q_filter.data_ptr())
        return ctypes.byref(desc), (desc, q_filter)


SEARCH_NAMES = ("filter", "q_filter", "a filter")   # what the messages call (the filter, its row picker, the thing picked from) ...
BASE_NAMES = ("base", "q_base", "a base filter")    # ... at a search door and at a row builder's door


def _checked(index, filter, q_filter, names):
    """The filter keyword of a door, checked against ``index``; None when neither keyword is given"""
    name, q_name, picked_from = names
    if filter is None:
        if q_filter is not None:
            raise ValueError(f"{q_name} picks rows of {picked_from}: it needs {name}=")
        return None
    if not isinstance(filter, DocFilter):
        raise ValueError(f"{name} must be a DocFilter")
    return filter.for_index(index)


def resolve_filter(index, filter, q_filter, nq: int, names=SEARCH_NAMES):
    """What the device doors do with their ``filter`` / ``q_filter`` (a row builder: ``base`` / ``q_base``) keywords: (None, None)
    when there is no filter, else (pointer to the call's struct, keep-alive)."""
    f = _checked(index, filter, q_filter, names)
    return (None, None) if f is None else f.launch_args(q_filter, nq)


def host_q_filter(index, filter, q_filter, nq: int, names=SEARCH_NAMES):
    """What the host-array doors do with the same keywords: the host ``q_filter`` validated (:func:`validate_q_filter`) and
    uploaded for the device door; None without a filter, and for None"""
    f = _checked(index, filter, q_filter, names)
    return None if f is None else q_filter_to_device(f, q_filter, nq)


def q_filter_to_device(filter: DocFilter, q_filter, nq: int):
    """A host ``q_filter`` validated (:func:`validate_q_filter`) and uploaded; None stays None."""
    q = validate_q_filter(q_filter, nq, filter.n_filters)
    return None if q is None else _torch().as_tensor(q, device=filter.device)


# -- the door of the row builders (DeviceIndex.term_filter_device, FieldTable.filter_device) ---------------------------------------
def builder_lists(device, lists, ids: str):
    """The ``all`` / ``any`` / ``none`` keywords of a row builder -- each None or a ``(ptr, ids)`` pair of 1-D int32 tensors on
    ``device``, a CSR over the output rows -- as (n_rows, the six tensors in the order the C entry points take them; None: list not
    given).  An empty id tensor is passed as a one-element placeholder (the entry points take "ptr and ids, both or neither").
    ``ids``: the word the messages have for the second tensor ("term", "clause").  ValueError: a pair that is not such tensors,
    lists that disagree on the row count, no list, no row."""
    torch = _torch()
    n_rows, tensors = None, []
    for name, pair in zip(("all", "any", "none"), lists):
        if pair is None:
            tensors += [None, None]
            continue
        ptr, row_ids = pair
        for t in (ptr, row_ids):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.device != device or t.dim() != 1:
                raise ValueError(f"{name} must be a (ptr, {ids}) pair of 1-D int32 tensors on {device}")
        if ptr.numel() < 1 or (n_rows is not None and ptr.numel() - 1 != n_rows):
            raise ValueError(f"the {ids} lists must have one ptr entry per output row, plus one, and agree on the row count")
        n_rows = ptr.numel() - 1
        tensors += [ptr.contiguous(), row_ids.contiguous() if row_ids.numel() else torch.zeros(1, dtype=torch.int32, device=device)]
    if n_rows is None:
        raise ValueError("give at least one of all / any / none (an empty list is a ptr of zeros)")
    if n_rows < 1:
        raise ValueError("a filter needs at least one row")
    return n_rows, tensors


def build_rows(owner, entry: str, launch, lists, ids: str, base, q_base, out) -> DocFilter:
    """The door of a row builder, for ``owner`` (``device``, ``n_docs``, ``doc_base``: the sparse index, a field table):
    :func:`builder_lists`, the ``base`` / ``q_base`` keywords (:func:`resolve_filter`), ``out`` allocated or checked, then
    ``launch(n_rows, the six list pointers, the base struct or None, out's pointer, the current stream)`` -> the return code of
    the C entry point ``entry``.  Returns the DocFilter over ``out``."""
    torch = _torch()
    n_rows, tensors = builder_lists(owner.device, lists, ids)
    bdesc, keep = resolve_filter(owner, base, q_base, n_rows, BASE_NAMES)  # keep: alive until the call below has been issued
    with torch.cuda.device(owner.device):
        if out is None:
            out = torch.empty((n_rows, filter_words(owner.n_docs)), dtype=torch.int32, device=owner.device)
        f = DocFilter(out, owner.n_docs, owner.doc_base)
        if f.n_filters != n_rows or f.device != owner.device:
            raise ValueError(f"out must be an int32 tensor [{n_rows}, {f.words}] on {owner.device}")
        rc = launch(n_rows, [None if t is None else t.data_ptr() for t in tensors], bdesc, out.data_ptr(),
                    torch.cuda.current_stream(owner.device).cuda_stream)
        _capi.check(rc, entry)
    del keep
    return f
