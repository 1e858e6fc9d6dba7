"""Seeded noise, host side (no GPU): the numpy reference of the stream definition (tests/philox_ref.py) reproduces the Random123
known answers and has the moments of a normal sample; insv2v.rng.stream_id is injective, range-checked and independent of the world
size; header, ctypes mirror and CLI carry the ABI-14 entries."""
import itertools
import re

import numpy as np
import pytest

import philox_ref
from conftest import ROOT

SEED, STREAM, N = 0x0123456789ABCDEF, 7, 1 << 20


@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_reference_reproduces_the_random123_known_answers(counter, key, want):
    got = " ".join("%08x" % int(w[0]) for w in philox_ref.philox4x32_10(counter, key))
    assert got == want


def test_reference_key_counter_and_element_layout():
    # the first known answer through the stream interface; seed = -1 / stream = -1 are the all-ones key and high counter words
    assert ["%08x" % w for w in philox_ref.words(0, 0, 0, 4)] == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    ones = philox_ref.philox4x32_10((5, 0, 0xFFFFFFFF, 0xFFFFFFFF), (0xFFFFFFFF, 0xFFFFFFFF))
    assert philox_ref.words(-1, -1, 20, 4).tolist() == [int(w[0]) for w in ones]
    # element i = word i & 3 of block i >> 2: any sub-range equals the same range of a longer draw, across the 2^34 carry too
    long = philox_ref.words(SEED, STREAM, 0, 1000)
    assert np.array_equal(philox_ref.words(SEED, STREAM, 137, 763), long[137:900])
    edge = philox_ref.words(5, 9, 2 ** 34 - 6, 16)
    assert np.array_equal(edge[6:10], philox_ref.blocks(5, 9, 2 ** 32, 1)[0])
    z = philox_ref.normals(SEED, STREAM, 0, 1000)
    assert np.array_equal(philox_ref.normals(SEED, STREAM, 137, 763), z[137:900])


def test_reference_normals_have_normal_moments():
    got = philox_ref.check_moments(philox_ref.normals(SEED, STREAM, 0, N))
    print("[seeded noise] float64 reference moments:", got)
    assert got["max"] < 5.89


def test_stream_id_is_injective_and_range_checked():
    from insv2v.rng import stream_id, ENC, INIT, STEP
    units = (0, 1, 2, 255, 256, 2 ** 24 - 2, 2 ** 24 - 1)
    windows = (0, 1, 15, 16, 4094, 4095)
    steps = (0, 1, 19, 255, 256, 65534, 65535)
    ids = [stream_id(k, u, w, s) for k, u, w, s in itertools.product((ENC, INIT, STEP), units, windows, steps)]
    assert len(set(ids)) == len(ids)
    assert all(0 <= i < 2 ** 63 for i in ids)
    assert stream_id(STEP, 3) == stream_id(STEP, 3, 0, 0)
    for bad in ((STEP, 2 ** 24, 0, 0), (STEP, 0, 4096, 0), (STEP, 0, 0, 65536), (STEP, -1, 0, 0), (INIT, 0, -1, 0), (ENC, 0, 0, -1),
                (3, 0, 0, 0), (-1, 0, 0, 0), (STEP, 1.5, 0, 0)):
        with pytest.raises(ValueError):
            stream_id(*bad)


def test_stream_ids_do_not_depend_on_the_world_size():
    """The driver numbers units before shard_units deals them to the ranks: the (unit, stream ids) reachable are those of one rank."""
    from insv2v.rng import stream_id, ENC, INIT, STEP
    from insv2v.clip_parallel import shard_units

    def reachable(world, n=7):
        out = set()
        for rank in range(world):
            for unit in shard_units(n, rank, world):
                out.add((unit, stream_id(ENC, unit), stream_id(INIT, unit, 1), stream_id(STEP, unit, 1, 19)))
        return out
    assert reachable(1) == reachable(2) == reachable(3) and len(reachable(1)) == 7


def test_header_and_ctypes_mirror_carry_abi_15():
    import ctypes
    from insv2v import _lib
    header = open(ROOT + "/include/insv2v_hip.h").read()
    assert _lib.ABI_VERSION == 15
    for name in ("insv2v_randn", "insv2v_posterior_sample_seeded"):
        assert re.search(r"^int %s\(" % name, header, flags=re.M), name
        assert name in _lib.SIGNATURES
    assert _lib.SIGNATURES["insv2v_randn"][1] == [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                                  ctypes.c_int32, ctypes.c_void_p]
    tail = _lib.StepDesc._fields_[-3:]
    assert tail == [("noise_seed", ctypes.c_int64), ("noise_stream", ctypes.c_int64), ("noise_on", ctypes.c_int32)]
    assert re.search(r"int64_t noise_seed, noise_stream;\s*int32_t noise_on;", header)
    for word in ("0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85", "bits 52-53", "bits 28-51", "bits 16-27", "bits 0-15"):
        assert word in header, word


def test_cli_takes_a_seed():
    from insv2v.run_loveu_tgve import build_parser
    assert build_parser().parse_args([]).seed is None
    assert build_parser().parse_args(["--seed", "5"]).seed == 5


def test_as_int64_takes_the_two_complement_bits():
    from insv2v.rng import as_int64
    assert as_int64(-1) == -1 and as_int64(2 ** 64 - 1) == -1 and as_int64(2 ** 63) == -2 ** 63 and as_int64(SEED) == SEED
    for bad in (2 ** 64, -2 ** 63 - 1, 0.5):
        with pytest.raises(ValueError):
            as_int64(bad)
