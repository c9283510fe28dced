"""bench.py's command line (no GPU): a plain run keeps only the headline build's steps, --full
turns the other legs back on with their defaults, --steps is the number of timed steps."""
import sys

import pytest

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


LEGS = ("weak_seqs", "annot_queries", "recall", "matrix_seqs", "cli_seqs", "cli_queries", "finish", "mph")


def test_plain_run_is_the_headline_only(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "3")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, None)
    assert all(getattr(a, k) == 0 for k in LEGS) and a.no_cpu_baseline
    # a leg's own option does not bring the leg back without --full
    a = _parse(monkeypatch, "--weak-seqs", "100000", "--matrix-seqs", "20000")
    assert a.weak_seqs == 0 and a.matrix_seqs == 0


def test_full_keeps_every_leg_and_its_options(monkeypatch):
    a = _parse(monkeypatch, "--full", "--dump-outputs", "out")
    assert a.full and a.dump_outputs == "out"
    assert all(getattr(a, k) > 0 for k in LEGS) and not a.no_cpu_baseline
    a = _parse(monkeypatch, "--full", "--matrix-seqs", "0", "--no-cpu-baseline")
    assert a.matrix_seqs == 0 and a.no_cpu_baseline and a.weak_seqs == bench.C2_SEQS


@pytest.mark.parametrize("argv", [("--steps", "0"), ("--warmup", "-1")])
def test_steps_and_warmup_are_checked(monkeypatch, argv):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, *argv)
