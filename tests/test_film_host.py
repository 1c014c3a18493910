"""Host side of the progressive film (no GPU): the exported toColor thresholds,
the film entry points' argument checks, and the numpy restatement the GPU
tests compare the device film with (tests/film_helpers.py)."""
import ctypes

import numpy as np

from dsgpuraytracing_amd import native
from tests.film_helpers import FilmRestatement


def host_code(bits: np.ndarray) -> np.ndarray:
    """pt_to_color's code of the red channel for each float bit pattern."""
    bits = np.ascontiguousarray(bits, np.uint32)
    hdr = np.zeros((len(bits), 3), np.float32)
    hdr[:, 0] = bits.view(np.float32)
    frame = np.zeros(len(bits), np.uint32)
    native.check(native.lib().pt_to_color(hdr.ctypes.data, len(bits), 1, 0, 0, len(bits), 1, frame.ctypes.data))
    return frame & 0xFF


def test_to_color_thresholds_are_the_code_steps():
    thr = np.zeros(256, np.uint32)
    assert native.lib().pt_to_color_thresholds(thr.ctypes.data) == native.PT_OK
    assert thr[0] == 0
    assert (np.diff(thr.astype(np.int64)) > 0).all(), "thresholds must be strictly increasing"
    assert thr[255] <= 0x7F800000
    k = np.arange(1, 256)
    assert np.array_equal(host_code(thr[1:]), k)
    assert np.array_equal(host_code(thr[1:] - 1), k - 1)
    assert native.lib().pt_to_color_thresholds(None) == native.PT_E_INVALID


def test_film_entry_points_refuse_null_handles():
    L = native.lib()
    t = native.pt_tile(0, 0, 1, 1)
    out = ctypes.c_void_p()
    info = native.pt_film_info()
    buf = np.zeros(4, np.float32)
    calls = {
        "pt_film_create": lambda: L.pt_film_create(None, 4, 4, ctypes.byref(out)),
        "pt_film_clear": lambda: L.pt_film_clear(None, None),
        "pt_film_add_pass": lambda: L.pt_film_add_pass(None, ctypes.byref(t), 1, None),
        "pt_film_resolve_device": lambda: L.pt_film_resolve_device(None, None, None, None, None),
        "pt_film_resolve": lambda: L.pt_film_resolve(None, buf.ctypes.data, None, None),
        "pt_film_tile_error": lambda: L.pt_film_tile_error(None, ctypes.byref(t), 1, buf.ctypes.data),
        "pt_film_get_info": lambda: L.pt_film_get_info(None, ctypes.byref(info)),
        "pt_film_set_next_sample": lambda: L.pt_film_set_next_sample(None, 0),
        "pt_to_color_device": lambda: L.pt_to_color_device(None, None, 4, 4, 0, 0, 4, 4, None, None),
    }
    for name, call in calls.items():
        L.pt_set_params(None, None)  # (another message in pt_last_error first)
        assert call() == native.PT_E_INVALID, name
        assert name.encode() in L.pt_last_error(), (name, L.pt_last_error())
    assert out.value is None
    assert L.pt_film_destroy(None) == native.PT_OK


def test_restatement_error_matches_float64_two_pass():
    """The helper itself: its streaming float32 error estimate against the
    textbook two-pass weighted computation in float64 on random non-negative
    passes of unequal weights.  Observed maximum relative difference: 5.6e-5
    (float32 roundings of mu and of the K <= 12 M2 terms, amplified where a
    pixel's passes lie close together); bound: the larger of 64 x that and
    1e-4, i.e. 3.6e-3."""
    rng = np.random.default_rng(12)
    h, w = 24, 40
    observed = 5.6e-5
    worst = 0.0
    for K in (2, 3, 7, 12):
        film = FilmRestatement(w, h)
        spps = rng.integers(1, 9, K)
        ms = [(rng.random((h, w, 3)) * rng.random((h, w, 1)) * 4).astype(np.float32) for _ in range(K)]
        for m, s in zip(ms, spps):
            film.add_pass(m, int(s))
        wt = spps.astype(np.float64)[:, None, None]
        m64 = np.stack(ms).astype(np.float64)
        L = 0.2126 * m64[..., 0] + 0.7152 * m64[..., 1] + 0.0722 * m64[..., 2]
        n = wt.sum()
        mean = (wt * L).sum(axis=0) / n
        M2 = (wt * (L - mean) ** 2).sum(axis=0)
        ref = np.sqrt(M2 / n / (K - 1)) / np.maximum(mean, 1e-3)
        got = film.err().astype(np.float64)
        assert np.isfinite(got).all()
        assert np.allclose(film.hdr(), (wt[..., None] * m64).sum(axis=0) / n, rtol=1e-5, atol=0)
        worst = max(worst, float((np.abs(got - ref) / ref).max()))
    bound = max(64 * observed, 1e-4)
    assert worst <= bound, f"max relative difference {worst:.3e} > {bound:.3e}"
    print(f"restatement vs float64 two-pass: max relative difference {worst:.3e}")
