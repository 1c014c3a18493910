"""The film merge of include/ptgpu.h (pt_film_merge_device) restated in numpy
float32 on FilmRestatement objects, one elementwise operation per line: numpy
rounds each operation to float32 and never fuses two, and its `/` is correctly
rounded, so the device merge must agree with this bit for bit.  A film here
may carry a `pad` plane (the fourth word of the second record; absent = 0)."""
import numpy as np

from tests.film_helpers import F, FilmRestatement

PLANES = ("sum", "n", "mu", "M2", "k", "pad")
CLASSES = ("merged", "taken", "empty", "refused")


def pad_of(r: FilmRestatement) -> np.ndarray:
    if not hasattr(r, "pad"):
        r.pad = np.zeros(r.n.shape, np.uint32)
    return r.pad


def copy_film(r: FilmRestatement) -> FilmRestatement:
    h, w = r.n.shape
    out = FilmRestatement(w, h)
    pad_of(r), pad_of(out)
    for name in PLANES:
        getattr(out, name)[...] = getattr(r, name)
    return out


def records(r: FilmRestatement) -> np.ndarray:
    """The film's device layout (csrc/film.h): (2, H, W, 4) uint32."""
    h, w = r.n.shape
    rec = np.zeros((2, h, w, 4), np.uint32)
    rec[0, ..., :3] = np.ascontiguousarray(r.sum).view(np.uint32)
    rec[0, ..., 3] = r.n
    rec[1, ..., 0] = np.ascontiguousarray(r.mu).view(np.uint32)
    rec[1, ..., 1] = np.ascontiguousarray(r.M2).view(np.uint32)
    rec[1, ..., 2] = r.k
    rec[1, ..., 3] = pad_of(r)
    return rec


def from_records(rec: np.ndarray) -> FilmRestatement:
    rec = np.ascontiguousarray(rec).view(np.uint32)
    _, h, w, _ = rec.shape
    r = FilmRestatement(w, h)
    r.sum[...] = np.ascontiguousarray(rec[0, ..., :3]).view(F)
    r.n[...] = rec[0, ..., 3]
    r.mu[...] = np.ascontiguousarray(rec[1, ..., 0]).view(F)
    r.M2[...] = np.ascontiguousarray(rec[1, ..., 1]).view(F)
    r.k[...] = rec[1, ..., 2]
    pad_of(r)[...] = rec[1, ..., 3]
    return r


def classes(a: FilmRestatement, b: FilmRestatement) -> dict:
    """The (h, w) bool mask of each pixel class of a <- a (+) b."""
    empty = b.n == 0
    taken = ~empty & (a.n == 0)
    both = ~empty & ~taken
    fits = a.n.astype(np.uint64) + b.n.astype(np.uint64) < np.uint64(2 ** 32)
    return {"merged": both & fits, "taken": taken, "empty": empty, "refused": both & ~fits}


def merge(a: FilmRestatement, b: FilmRestatement) -> dict:
    """a <- a (+) b in place; returns the four class counts."""
    cls = classes(a, b)
    pad_of(a), pad_of(b)
    t = cls["taken"]
    for name in PLANES:
        getattr(a, name)[t] = getattr(b, name)[t]
    m = cls["merged"]
    s = a.sum[m] + b.sum[m]
    n = a.n[m] + b.n[m]
    W = n.astype(F)
    fa = a.n[m].astype(F)
    fb = b.n[m].astype(F)
    d = b.mu[m] - a.mu[m]
    r = fb / W
    u = d * r
    mu = a.mu[m] + u
    q = a.M2[m] + b.M2[m]
    dd = d * d
    ab = fa * fb
    g = ab / W
    v = dd * g
    M2 = q + v
    k = a.k[m] + b.k[m]
    a.sum[m] = s
    a.n[m] = n
    a.mu[m] = mu
    a.M2[m] = M2
    a.k[m] = k
    return {name: int(cls[name].sum()) for name in CLASSES}


def merge_records(rec_a: np.ndarray, rec_b: np.ndarray):
    """(records of a (+) b, the four counts) from two record arrays."""
    a = from_records(rec_a)
    counts = merge(a, from_records(rec_b))
    return records(a), counts
