"""The film merge as include/ptgpu.h defines it (pt_film_merge_device), on the
CPU: the numpy restatement (tests/film_merge_helpers.py) that the device
kernel is compared with bit for bit has the properties the definition
promises -- the trivial cases, the four pixel classes, the overflow refusal --
and a K + K merge is as close to the float64 statistics as the sequential 2K
pass film (existing code: FilmRestatement.add_pass) is."""
import numpy as np
import pytest

from tests.film_helpers import F, FilmRestatement, bits
from tests.film_merge_helpers import CLASSES, classes, copy_film, from_records, merge, merge_records, records

W, H = 64, 64


def synthetic_passes(count: int, seed: int = 7, w: int = W, h: int = H):
    """`count` pass images: a gamma-distributed luminance per pixel and pass
    times the pixel's tint, 30% of the pixels black in every pass."""
    rng = np.random.default_rng(seed)
    tint = (F(0.2) + F(0.8) * rng.random((h, w, 3))).astype(F)
    black = rng.random((h, w)) < 0.3
    out = []
    for _ in range(count):
        L = rng.gamma(2.0, 0.25, (h, w)).astype(F)
        m = (L[..., None] * tint).astype(F)
        m[black] = 0
        out.append(m)
    return out


def film_of(passes, spp: int, mask=None, w: int = W, h: int = H) -> FilmRestatement:
    r = FilmRestatement(w, h)
    for m in passes:
        r.add_pass(m, spp, mask)
    return r


def same_film(a, b) -> bool:
    return np.array_equal(records(a), records(b))


def luminance(m):
    a = F(0.2126) * m[..., 0]
    b = F(0.7152) * m[..., 1]
    c = F(0.0722) * m[..., 2]
    return (a + b) + c


def test_trivial_cases_and_counts():
    ps = synthetic_passes(3)
    film, empty = film_of(ps, 2), FilmRestatement(W, H)
    before = copy_film(film)
    assert merge(film, empty) == {"merged": 0, "taken": 0, "empty": W * H, "refused": 0}
    assert same_film(film, before)
    into = FilmRestatement(W, H)
    into.pad = np.full((H, W), 5, np.uint32)  # (a clear pixel's pad goes too: both records become b's)
    film.pad = np.arange(W * H, dtype=np.uint32).reshape(H, W)
    assert merge(into, film) == {"merged": 0, "taken": W * H, "empty": 0, "refused": 0}
    assert same_film(into, film)
    # the records round trip, and a partly covered pair has three classes that sum to W * H
    assert same_film(from_records(records(film)), film)
    left = np.zeros((H, W), bool)
    left[:, :40] = True
    right = np.zeros((H, W), bool)
    right[:, 24:56] = True
    a, b = film_of(ps[:2], 3, left), film_of(ps[2:], 1, right)
    pad_a = a.pad = np.full((H, W), 9, np.uint32)
    b.pad = np.full((H, W), 4, np.uint32)
    c = merge(a, b)
    assert c == {"merged": H * 16, "taken": H * 16, "empty": H * 32, "refused": 0} and sum(c.values()) == W * H
    assert (a.pad[:, :40] == 9).all() and (a.pad[:, 40:56] == 4).all() and pad_a is a.pad  # merged keeps a's pad
    assert (a.k[:, 24:40] == 3).all() and (a.n[:, 24:40] == 7).all()


def test_overflow_is_refused():
    a = film_of(synthetic_passes(2, w=8, h=2), 1, w=8, h=2)
    b = film_of(synthetic_passes(1, seed=3, w=8, h=2), 1, w=8, h=2)
    top = 2 ** 32 - 1
    a.n[0] = [top, top - 1, top - 2, 1, 2 ** 31, 2 ** 31, 2 ** 31 - 1, 0]
    b.n[0] = [1, 1, 1, top, 2 ** 31, 2 ** 31 - 1, 2 ** 31, top]
    refused = np.array([1, 0, 0, 1, 1, 0, 0, 0], bool)
    before = copy_film(a)
    cls = classes(a, b)
    assert np.array_equal(cls["refused"][0], refused) and not cls["refused"][1].any() and cls["taken"][0, 7]
    c = merge(a, b)
    assert c["refused"] == 3 and c["taken"] == 1 and sum(c.values()) == 16
    rec, rec0 = records(a), records(before)
    assert np.array_equal(rec[:, 0, refused], rec0[:, 0, refused])
    assert (a.n[0, ~refused] == top - np.array([0, 1, 0, 0, 0])).all()
    # the same through the record arrays
    got, c2 = merge_records(rec0, records(b))
    assert np.array_equal(got, rec) and c2 == c


# (K, spp): merged / sequential deviation from float64 measured for mu, M2 and
# the sum's difference as a share of its bound:
#   (8, 1) 0.77 0.60 0.12   (8, 4) 0.77 0.60 0.12   (32, 2) 0.55 0.64 0.06   (3, 5) 0.86 1.34 0.27
@pytest.mark.parametrize("K,spp", [(8, 1), (8, 4), (32, 2), (3, 5)])
def test_merge_is_as_accurate_as_the_sequential_film(K, spp):
    """2K passes: a K + K merge against the sequential 2K-pass film and the
    float64 values of the same passes.  n and k exactly; the sums within the
    bound of two summation orders of the same 2K non-negative f32 terms; mu
    and M2 deviate from float64 at most twice as far as the sequential film's
    own (two Welford chains of length K plus one combine against one chain of
    length 2K)."""
    ps = synthetic_passes(2 * K)
    seq = film_of(ps, spp)
    mrg = film_of(ps[:K], spp)
    counts = merge(mrg, film_of(ps[K:], spp))
    assert counts == {"merged": W * H, "taken": 0, "empty": 0, "refused": 0}
    assert np.array_equal(mrg.n, seq.n) and np.array_equal(mrg.k, seq.k)
    assert (seq.n == 2 * K * spp).all() and (seq.k == 2 * K).all()
    L = np.stack([luminance(m) for m in ps]).astype(np.float64)
    mu64 = (spp * L).sum(0) / (2 * K * spp)
    M264 = (spp * (L - mu64) ** 2).sum(0)
    sum64 = sum(spp * m.astype(np.float64) for m in ps)
    bound = 2 * (2 * K) * 2.0 ** -24 * sum64
    diff = np.abs(mrg.sum.astype(np.float64) - seq.sum.astype(np.float64))
    dev = {name: [np.abs(getattr(f, name).astype(np.float64) - ref).max() for f in (mrg, seq)]
           for name, ref in (("mu", mu64), ("M2", M264))}
    print(f"K {K} spp {spp}: mu {dev['mu'][0] / dev['mu'][1]:.2f} M2 {dev['M2'][0] / dev['M2'][1]:.2f} "
          f"sum {(diff[bound > 0] / bound[bound > 0]).max():.2f}")
    assert (diff <= bound).all()
    for name, (d_mrg, d_seq) in dev.items():
        assert d_seq > 0 and d_mrg <= 2 * d_seq, (name, d_mrg, d_seq)
    assert not np.array_equal(bits(mrg.mu), bits(seq.mu))  # (another rounding order, not the same film)


def test_merge_is_not_bitwise_commutative_but_disjoint_merges_are():
    ps = synthetic_passes(6)
    a, b = film_of(ps[:3], 2), film_of(ps[3:], 3)
    ab, ba = copy_film(a), copy_film(b)
    merge(ab, b), merge(ba, a)
    assert np.array_equal(ab.n, ba.n) and np.array_equal(ab.k, ba.k)
    assert not np.array_equal(bits(ab.mu), bits(ba.mu))  # hence the fixed order (ptgpu.h)
    assert np.allclose(ab.mu, ba.mu, rtol=1e-5, atol=1e-7) and np.allclose(ab.M2, ba.M2, rtol=1e-4, atol=1e-6)
    even = np.zeros((H, W), bool)
    even[::2] = True
    x, y = film_of(ps, 2, even), film_of(ps, 2, ~even)
    xy, yx = copy_film(x), copy_film(y)
    cx, cy = merge(xy, y), merge(yx, x)
    assert cx == cy == {"merged": 0, "taken": W * H // 2, "empty": W * H // 2, "refused": 0}
    assert same_film(xy, yx) and same_film(xy, film_of(ps, 2))
    assert set(cx) == set(CLASSES)
