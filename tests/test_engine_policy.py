"""The engine's pure decisions (gdv_engine_policy.h) compiled for the HOST with g++ alone (tests/host_engine_policy/):
which kernels a var-len batch starts on and moves to, and how big the temporaries of a two-stage plan start.
The whole table is walked against the rules as Projector::LaunchVarlen's comment states them; no GPU."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_engine_policy", "host_engine_policy.cc")
LIB = os.path.join(HERE, "host_engine_policy", "libhost_engine_policy.so")
HDR = os.path.join(HERE, "..", "gandiva_amd", "csrc", "gdv_engine_policy.h")

NOTFLAT, NOTASCII, SAWUTF8 = 16, 32, 64


@pytest.fixture(scope="module")
def policy():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-Wall", "-Werror", SRC, "-o", LIB])
    lib = C.CDLL(LIB)
    for f in (lib.host_stage_capacity, lib.host_stage_guess_max):
        f.restype = C.c_longlong
    lib.host_stage_capacity.argtypes = [C.c_longlong] * 3
    return lib


def test_the_status_bits_are_the_device_librarys(policy):
    assert policy.host_status_bits() == NOTFLAT | NOTASCII << 8 | SAWUTF8 << 16
    devlib = open(os.path.join(os.path.dirname(HDR), "gdv_device_lib.hpp")).read()
    for name, bit in (("GDV_ERR_NOTFLAT", NOTFLAT), ("GDV_ERR_NOTASCII", NOTASCII), ("GDV_ERR_SAWUTF8", SAWUTF8)):
        assert f"#define {name} {bit}u" in devlib


@pytest.mark.parametrize("hint,has_optimistic,has_exact,no_optflat,counter",
                         list(itertools.product((0, 1, 2), (False, True), (False, True), (False, True), (14, 15))))
def test_the_path_a_var_len_batch_starts_on(policy, hint, has_optimistic, has_exact, no_optflat, counter):
    if not has_optimistic:
        base = 2                       # one kernel only, scanner-shaped
    elif no_optflat:
        base = 2                       # GDV_NO_OPTFLAT: straight to the general kernel
    else:
        base = hint                    # where the last batch left the projector ...
        if base == 1 and not has_exact:
            base = 2                   # ... the exact variant only where the plan has one
    # the optimistic kernels get another try on every 16th batch that would start on the general kernel
    retry = base == 2 and has_optimistic and not no_optflat and counter == 15
    assert policy.host_varlen_start_path(hint, has_optimistic, has_exact, no_optflat, counter) == (0 if retry else base)
    # a caller that never retries (the asynchronous entry) passes 0
    assert policy.host_varlen_start_path(hint, has_optimistic, has_exact, no_optflat, 0) == base


@pytest.mark.parametrize("bits", [sum(c) for k in range(4) for c in itertools.combinations((NOTFLAT, NOTASCII, SAWUTF8), k)])
@pytest.mark.parametrize("has_exact", [False, True])
def test_the_path_after_a_launch(policy, bits, has_exact):
    # after the optimistic attempt: NOTASCII -> the exact variant; NOTFLAT (with or without NOTASCII), or NOTASCII
    # on a plan without an exact variant -> the general kernel; neither -> done
    if bits & NOTASCII and not bits & NOTFLAT and has_exact:
        want0 = 1
    elif bits & (NOTASCII | NOTFLAT):
        want0 = 2
    else:
        want0 = 0
    assert policy.host_varlen_next_path(0, bits, has_exact) == want0
    # after the exact variant: NOTFLAT -> the general kernel; anything else (SAWUTF8 is a note, not an error) -> done
    assert policy.host_varlen_next_path(1, bits, has_exact) == (2 if bits & NOTFLAT else 1)
    # the general kernel is the last resort
    assert policy.host_varlen_next_path(2, bits, has_exact) == 2


def test_stage_capacity(policy):
    rows, guess = 1000, 32 * 1000 + 5000
    assert policy.host_stage_capacity(guess, 0, rows) == guess                # no batch yet: the blanket guess
    # 4 bytes per row seen (x 16 = 64): 4000 bytes + 25 % + 4096 = 9096 caps below the guess
    assert policy.host_stage_capacity(guess, 64, rows) == 9096
    # 40 bytes per row seen: 40000 + 25 % + 4096 would cap above the guess — the guess holds
    assert policy.host_stage_capacity(guess, 640, rows) == guess
    assert policy.host_stage_capacity(0, 640, rows) == 0                       # (host buffers start from nothing)
    assert policy.host_stage_guess_max() == 2**31 - 64
