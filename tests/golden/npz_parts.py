"""Fixtures larger than a committed file may be (1 MiB) are stored as NAME_part<k>.npz, each a compressed npz of whole groups of
keys ("<group>/..."); load() merges them back into one mapping.  Pure data handling: no reference code is involved."""
import glob
import io
import os

import numpy as np

PART_BYTES = 900 * 1024


def _parts(path):
    stem = path[:-len(".npz")]
    return sorted(glob.glob(stem + "_part*.npz"), key=lambda p: int(p[len(stem) + len("_part"):-len(".npz")]))


def load(path):
    """The arrays of PATH (a .npz), or of its parts NAME_part1.npz, NAME_part2.npz, ... merged: a dict name -> array."""
    if os.path.exists(path):
        with np.load(path) as z:
            return {k: z[k] for k in z.files}
    parts = _parts(path)
    if not parts:
        raise FileNotFoundError(path)
    out = {}
    for p in parts:
        with np.load(p) as z:
            out.update({k: z[k] for k in z.files})
    return out


def _size(arrays):
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    return buf.tell()


def save(path, arrays, limit=PART_BYTES):
    """Write ARRAYS as PATH when it compresses to at most `limit` bytes, else as parts of whole key groups (the text before the
    first "/") of at most `limit` bytes each; stale parts or a stale whole file of the same name are removed."""
    for p in _parts(path) + ([path] if os.path.exists(path) else []):
        os.remove(p)
    if _size(arrays) <= limit:
        np.savez_compressed(path, **arrays)
        return [path]
    groups = {}
    for k, v in arrays.items():
        groups.setdefault(k.split("/", 1)[0], {})[k] = v
    parts, cur = [], {}
    for g in groups.values():
        if cur and _size(dict(cur, **g)) > limit:
            parts.append(cur)
            cur = {}
        cur.update(g)
    parts.append(cur)
    stem, paths = path[:-len(".npz")], []
    for i, p in enumerate(parts, 1):
        assert _size(p) <= limit, "one key group of %s is larger than %d bytes" % (path, limit)
        paths.append("%s_part%d.npz" % (stem, i))
        np.savez_compressed(paths[-1], **p)
    return paths
