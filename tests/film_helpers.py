"""The film arithmetic of include/ptgpu.h (pt_film_add_pass / pt_film_resolve)
restated in numpy float32, one elementwise operation per line: numpy rounds
each operation to float32 and never fuses two, and its `/` and np.sqrt are
correctly rounded, so the device film must agree with this bit for bit."""
import numpy as np

F = np.float32
LUM_FLOOR = F(1e-3)  # PT_FILM_LUM_FLOOR


class FilmRestatement:
    def __init__(self, w: int, h: int):
        self.sum = np.zeros((h, w, 3), F)
        self.n = np.zeros((h, w), np.uint32)
        self.mu = np.zeros((h, w), F)
        self.M2 = np.zeros((h, w), F)
        self.k = np.zeros((h, w), np.uint32)

    def add_pass(self, m: np.ndarray, spp: int, mask=None):
        """m: the pass image (h, w, 3) float32; mask: (h, w) bool of the pixels
        inside the pass's tiles (None: the whole frame)."""
        assert m.dtype == F
        if mask is None:
            mask = np.ones(self.n.shape, bool)
        w = F(spp)
        m = m[mask]
        s = self.sum[mask]
        t = m * w
        s = s + t
        n = self.n[mask] + np.uint32(spp)
        a = F(0.2126) * m[:, 0]
        b = F(0.7152) * m[:, 1]
        c = F(0.0722) * m[:, 2]
        L = a + b
        L = L + c
        W = n.astype(F)
        mu = self.mu[mask]
        d = L - mu
        r = w / W
        u = d * r
        mu = mu + u
        wd = w * d
        e = L - mu
        v = wd * e
        M2 = self.M2[mask] + v
        self.sum[mask] = s
        self.n[mask] = n
        self.mu[mask] = mu
        self.M2[mask] = M2
        self.k[mask] = self.k[mask] + np.uint32(1)

    def hdr(self) -> np.ndarray:
        out = np.zeros_like(self.sum)
        r = self.n > 0
        out[r] = self.sum[r] / self.n[r].astype(F)[:, None]
        return out

    def err(self) -> np.ndarray:
        out = np.full(self.n.shape, np.inf, F)
        r = self.k >= 2
        m2 = np.fmax(self.M2[r], F(0))
        q = m2 / self.n[r].astype(F)
        q = q / (self.k[r] - np.uint32(1)).astype(F)
        q = np.sqrt(q)
        out[r] = q / np.fmax(self.mu[r], LUM_FLOOR)
        return out


def tile_mask(w: int, h: int, tiles) -> np.ndarray:
    """(h, w) bool: the pixels of the tiles (x, y, tw, th), clipped to the frame."""
    m = np.zeros((h, w), bool)
    for (x, y, tw, th) in tiles:
        m[max(y, 0):max(min(y + th, h), 0), max(x, 0):max(min(x + tw, w), 0)] = True
    return m


def tile_max(err: np.ndarray, tiles) -> np.ndarray:
    """Per tile the maximum of the error plane over the clipped tile (0 when empty)."""
    h, w = err.shape
    out = np.zeros(len(tiles), F)
    for i, (x, y, tw, th) in enumerate(tiles):
        sub = err[max(y, 0):max(min(y + th, h), 0), max(x, 0):max(min(x + tw, w), 0)]
        out[i] = sub.max() if sub.size else F(0)
    return out


def bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a, F).view(np.uint32)
