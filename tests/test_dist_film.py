"""Joining the films of a split render (dist.FilmExchange and the two split
drivers) over gloo on the CPU: numpy records and the restatement merge stand in
for the device films (tests/test_gpu_film_merge.py runs the same calls on
them).  The root's film must equal the other ranks' records merged in rank
order, bit for bit -- the merge is not commutative -- and the drivers' sample
ranges must tile [0, world * passes * spp) without a gap."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from dsgpuraytracing_amd.dist import (FilmExchange, film_passes_sample_split, film_passes_tile_split, shard_tiles)
from dsgpuraytracing_amd.pathtracer import tile_fifo
from tests.film_helpers import F, FilmRestatement
from tests.film_merge_helpers import from_records, merge, records

W, H = 40, 24


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def rank_film(rank: int) -> FilmRestatement:
    """Rank r's film: r + 2 passes of r + 1 samples over all but the columns
    8r .. 8r + 7, so the ranks' films overlap and every class but `refused`
    occurs."""
    rng = np.random.default_rng(100 + rank)
    mask = np.ones((H, W), bool)
    mask[:, 8 * rank:8 * rank + 8] = False
    r = FilmRestatement(W, H)
    for _ in range(rank + 2):
        r.add_pass(rng.gamma(2.0, 0.25, (H, W, 3)).astype(F), rank + 1, mask)
    return r


def as_tensor_export(film):
    def export(buf):
        buf.copy_(torch.from_numpy(records(film).view(np.int32)))
    return export


def _worker(rank, world, port, out_path):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    film = rank_film(rank)
    before = records(film).copy()
    counts = []

    def merge_in(buf):
        counts.append(merge(film, from_records(buf.numpy().view(np.uint32))))

    ex = FilmExchange(W, H, rank, world, "cpu")
    ex.merge_to_root(as_tensor_export(film), merge_in)
    ok = len(counts) == (world - 1 if rank == 0 else 0)
    if rank == 0:
        np.savez(out_path, records=records(film), merged=[c["merged"] for c in counts])
    else:
        ok = ok and np.array_equal(records(film), before) and ex.recv is None
    flag = torch.tensor([0 if ok else 1], dtype=torch.int32)
    dist.all_reduce(flag, op=dist.ReduceOp.MAX)
    dist.destroy_process_group()
    assert int(flag.item()) == 0


@pytest.mark.parametrize("world", [2, 3])
def test_merge_to_root_in_rank_order(tmp_path, world):
    out = str(tmp_path / "root.npz")
    mp.spawn(_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    want = rank_film(0)
    merged = [merge(want, rank_film(r))["merged"] for r in range(1, world)]
    with np.load(out) as z:
        assert np.array_equal(z["records"], records(want))
        assert z["merged"].tolist() == merged and all(m > 0 for m in merged)
    if world == 3:  # the order matters: 0 (+) 2 (+) 1 is another film
        other = rank_film(0)
        merge(other, rank_film(2)), merge(other, rank_film(1))
        assert not np.array_equal(records(other), records(want))
        assert np.array_equal(other.n, want.n)


def test_one_rank_does_nothing_and_many_need_a_group():
    assert not dist.is_initialized()
    film = rank_film(0)
    calls = []
    ex = FilmExchange(W, H, 0, 1, "cpu")
    ex.merge_to_root(lambda buf: calls.append("export"), lambda buf: calls.append("merge"))
    assert calls == [] and ex.recv is None
    # the gather alone still hands the records over (no group: a copy)
    got = ex.gather(as_tensor_export(film))
    assert np.array_equal(got[0].numpy().view(np.uint32), records(film))
    ex2 = FilmExchange(W, H, 1, 2, "cpu")
    with pytest.raises(RuntimeError, match="process group"):
        ex2.merge_to_root(as_tensor_export(film), lambda buf: calls.append("merge"))
    assert calls == []
    with pytest.raises(ValueError):
        FilmExchange(W, H, 2, 2, "cpu")


class FakeFilm:
    """What the drivers use of a pathtracer.Film; every pass draws `spp` samples."""

    def __init__(self, spp: int, next_sample: int = 0):
        self.spp, self.next = spp, next_sample
        self.passes = []  # (first sample, tiles)

    def set_next_sample(self, n):
        assert 0 <= n < 2 ** 32
        self.next = n

    def add_pass(self, tiles, stream=0):
        assert self.next + self.spp <= 2 ** 32
        self.passes.append((self.next, list(tiles)))
        self.next += self.spp

    def info(self):
        return {"next_sample": self.next}


@pytest.mark.parametrize("world", [1, 2, 3, 4])
def test_sample_split_ranges(world):
    tiles, passes, spp = tile_fifo(70, 37), 4, 3
    ranges = []
    for rank in range(world):
        film = FakeFilm(spp, next_sample=777)
        ranges.append(film_passes_sample_split(film, tiles, passes, spp, rank, world))
        assert [p[0] for p in film.passes] == [ranges[-1][0] + i * spp for i in range(passes)]
        assert all(p[1] == tiles for p in film.passes)
    assert ranges[0][0] == 0 and ranges[-1][1] == world * passes * spp
    assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))  # disjoint and contiguous
    # the params hold another spp than the driver was told
    with pytest.raises(RuntimeError, match="spp"):
        film_passes_sample_split(FakeFilm(spp + 1), tiles, passes, spp, 0, world)


def test_sample_split_refuses_beyond_the_sample_range():
    tiles = tile_fifo(32, 32)
    spp, passes = 2 ** 20, 2 ** 10  # one rank's share: 2^30 samples
    for rank in range(4):  # four shares are exactly 2^32: allowed (not run: no pass of a fake film costs anything)
        film = FakeFilm(spp)
        assert film_passes_sample_split(film, tiles, passes, spp, rank, 4) == (rank * 2 ** 30, (rank + 1) * 2 ** 30)
    for rank in (0, 4):  # five would pass it: refused on every rank, before anything is touched
        film = FakeFilm(spp, next_sample=5)
        with pytest.raises(ValueError, match="2\\^32"):
            film_passes_sample_split(film, tiles, passes, spp, rank, 5)
        assert film.passes == [] and film.next == 5
    with pytest.raises(ValueError):
        film_passes_sample_split(FakeFilm(1), tiles, 1, 0, 0, 1)
    with pytest.raises(ValueError):
        film_passes_sample_split(FakeFilm(1), tiles, 1, 1, 2, 2)


@pytest.mark.parametrize("world", [1, 2, 3])
def test_tile_split_shares(world):
    tiles, passes, spp = tile_fifo(96, 80), 3, 2
    seen = []
    for rank in range(world):
        film = FakeFilm(spp, next_sample=10)
        mine = film_passes_tile_split(film, tiles, passes, rank, world, spp=spp)
        assert mine == shard_tiles(tiles, rank, world)
        # every rank draws the same sample indices, for its own tiles only
        assert film.passes == [(10 + i * spp, mine) for i in range(passes)]
        seen += mine
    assert sorted(seen) == sorted(tiles)
    film = FakeFilm(4, next_sample=2 ** 32 - 11)
    with pytest.raises(ValueError, match="2\\^32"):
        film_passes_tile_split(film, tiles, 3, 0, 2, spp=4)
    assert film.passes == []
    assert film_passes_tile_split(FakeFilm(4, next_sample=2 ** 32 - 12), tiles, 3, 0, 2, spp=4)
