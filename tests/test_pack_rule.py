"""Packed small-n mode, the part that needs no GPU: the psg_pack_width rule, the psg_config.pack
field (the former `reserved`: same offset, same struct size) and the Python keywords."""
import ctypes as C
import os
import subprocess

import pytest

from round_amd import abi, lib, psync

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALGS = sorted(abi.CLASS_TO_ALG.values())


def otr_width(n):
    """G = 64 / P, P the power of two >= n, at least 4; no packing above n = 32."""
    if n > 32:
        return 1
    p = 4
    while p < n:
        p *= 2
    return 64 // p


def test_the_eleven_algorithms():
    assert ALGS == list(range(1, 12))


def test_otr_width_table():
    table = {n: lib.pack_width(abi.PSG_ALG_OTR, n) for n in range(1, abi.PSG_MAX_N + 1)}
    assert table == {n: otr_width(n) for n in range(1, abi.PSG_MAX_N + 1)}
    # the rows of the table as the header states them
    assert [table[n] for n in (1, 4, 5, 8, 9, 16, 17, 32, 33, 256)] == [16, 16, 8, 8, 4, 4, 2, 2, 1, 1]


@pytest.mark.parametrize("alg", [a for a in ALGS if a != abi.PSG_ALG_OTR])
def test_other_algorithms_are_not_packed(alg):
    assert [lib.pack_width(alg, n) for n in range(1, abi.PSG_MAX_N + 1)] == [1] * abi.PSG_MAX_N


@pytest.mark.parametrize("alg,n", [(0, 4), (99, 4), (abi.PSG_ALG_OTR, 0), (abi.PSG_ALG_OTR, 257)])
def test_width_rejects_unknown_algorithm_and_n(alg, n):
    assert lib.load().psg_pack_width(alg, n) == abi.PSG_EINVAL
    with pytest.raises(lib.PsgError):
        lib.pack_width(alg, n)


def test_pack_field_takes_the_reserved_slot():
    assert abi.Config.pack.offset == abi.Config.param2.offset + 4
    assert abi.Config.pack.size == 4
    assert abi.Config.real_param.offset == abi.Config.pack.offset + 4
    assert abi.PSG_ABI_VERSION == 4


def test_config_default_leaves_pack_off():
    L = lib.load()
    for alg in ALGS:
        c = abi.Config()
        c.pack = 7
        assert L.psg_config_default(C.byref(c), alg, 4) == 0
        assert c.pack == 0


def test_make_config_keyword():
    assert psync.make_config(psync.OTR(), 4).pack == 0
    assert psync.make_config(psync.OTR(), 4, pack=False).pack == 0
    assert psync.make_config(psync.OTR(), 4, pack=True).pack == 1
    assert psync.make_config(psync.LastVoting(), 5, pack=True).pack == 1
    # nothing else moves
    a, b = psync.make_config(psync.OTR(), 4), psync.make_config(psync.OTR(), 4, pack=True)
    b.pack = 0
    assert bytes(a) == bytes(b)


PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "psg.h"
int main(void) {
  psg_config c;
  printf("%zu %zu %zu %zu %zu\n", sizeof(psg_config), offsetof(psg_config, param2), offsetof(psg_config, pack),
         sizeof(c.pack), offsetof(psg_config, real_param));
  return 0;
}
"""


def test_c_struct_size_is_unchanged(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, param2, pack, pack_size, real_param = map(int, subprocess.check_output([str(exe)], text=True).split())
    # 56 bytes up to sched + 24 (sched) + param2, pack, real_param, n_devices, devices[16]: ABI version 4's 168 bytes
    assert size == C.sizeof(abi.Config) == 168
    assert (param2, pack, pack_size, real_param) == (abi.Config.param2.offset, abi.Config.pack.offset, 4,
                                                     abi.Config.real_param.offset)
