"""Group files of the grouped AUC (ops/kernels.py ``gauc``): one key per line (a user, a query, a session id:
any text, compared byte for byte after stripping the line end), one line per example, parallel to the data
files the way weight files are."""

from __future__ import annotations

import numpy as np


class GroupIndex:
    """Dense int32 group ids of the examples of some data files, in order of first appearance of their keys.

    ``ids[i]``: the group of example i, in ``[0, num_groups)``; ``keys[g]``: the key string of group g."""

    __slots__ = ("ids", "keys")

    def __init__(self, ids: np.ndarray, keys: list[str]):
        self.ids, self.keys = ids, keys

    @property
    def num_groups(self) -> int:
        return len(self.keys)


def _count_lines(path: str) -> int:
    with open(path, "rb") as f:
        return len(f.read().splitlines())


def load_group_files(group_files: list[str], data_files: list[str]) -> GroupIndex:
    """The groups of all lines of ``data_files`` (in order) from the parallel ``group_files``.  Every group
    file must have as many lines as its data file: a mismatch is a ``ValueError`` that names both."""
    if len(group_files) != len(data_files):
        raise ValueError("The numbers of data files and group files do not match.")
    index: dict[bytes, int] = {}
    ids: list[int] = []
    for gpath, dpath in zip(group_files, data_files):
        with open(gpath, "rb") as f:
            lines = f.read().splitlines()
        n = _count_lines(dpath)
        if len(lines) != n:
            raise ValueError(f"{gpath}: {len(lines)} lines but {dpath} has {n}")
        for key in lines:
            ids.append(index.setdefault(key.strip(), len(index)))
    if len(index) >= 2**31:
        raise ValueError("group files: more than 2^31 - 1 distinct keys")
    return GroupIndex(np.asarray(ids, dtype=np.int32), [k.decode("utf-8", "replace") for k in index])
