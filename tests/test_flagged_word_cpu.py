"""CPU: the host half of the flagged-word protocol (mimosa_amd/csrc/flagged_word.hpp, compiled by g++ through
tests/cpp/flagged_word.cpp): what the host accepts of a word, and the bounded spin.

Bars.  Acceptance and the returned bits: exact.  The spin with a budget <= 0 looks once and does not wait.  With a 1 ms budget and a
predicate that never holds it gives up after the budget and within 100 ms — two orders of magnitude of room for a loaded machine;
the helper reads the clock every 1024 spins, microseconds apart."""
import json
import subprocess

import pytest


@pytest.fixture(scope="module")
def got():
    from mimosa_amd import build
    out = subprocess.run([build.build_host_test("flagged_word")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return json.loads(out.stdout)


def test_halves_of_different_calls_are_refused(got):
    assert got["torn_a"] == 0 and got["torn_b"] == 0
    assert got["untouched"] == 1


def test_word_of_an_earlier_call_is_refused(got):
    assert got["stale"] == 0
    assert got["untouched"] == 1


def test_matching_word_returns_the_stored_bits(got):
    assert len(got["exact"]) == 10 and all(v == 1 for v in got["exact"])


def test_spin_without_budget_returns_at_once(got):
    assert got["looks_zero"] == 1 and got["looks_negative"] == 1
    assert 0.0 <= got["ms_zero"] < 100.0 and 0.0 <= got["ms_negative"] < 100.0  # (-1: the helper claimed the predicate held)


def test_spin_gives_up_after_its_budget(got):
    assert 1.0 <= got["ms_1ms"] < 100.0
    assert got["looks_1ms"] > 1
    assert got["holds"] == 1 and got["looks_holds"] == 3
