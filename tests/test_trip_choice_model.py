"""What the next trip of the wavefront kernel's traversal loop is (csrc/trip_choice.h), checked without a GPU.

tests/trip_choice_model.cpp compiles the header with the host compiler beside the forms the kernel had before it, copied as the
specification, and plays both:
- choice: every (n_t, n_i, n_p) with n_t + n_i + n_p <= 64, for the bounds 1, 64, 320, 512 and 768, at every debt from 0 to
  bound + 64 the loop can hold where it asks (the debt before this trip's n_p was below the bound: the loop leaves on the
  first trip that finds it there and a pass zeroes it) - leave / pass / step must be the same;
- masks: any_lane over lane masks, edge patterns and random ones;
- sequence: random runs of surveys from a reset debt - the sequence of choices must be the same, the first trip after a pass
  included;
- bound: a wait-debt bound of 0 is refused where the bound is made (kernel_choice.h), the bounds choose_wavefront makes run.
"""
import os
import re
import subprocess

import pytest

import model_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opencl_pathtracer_amd", "csrc")
MODEL_SRC = os.path.join(ROOT, "tests", "trip_choice_model.cpp")


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return model_build.program([MODEL_SRC], tmp_path_factory.mktemp("trip_choice"), "trip_choice_model", opt="-O1", werror=True,
                               includes=[CSRC, os.path.join(ROOT, "include")])


def run(model, *args):
    r = subprocess.run([model, *args], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-500:]
    return dict(zip(r.stdout.split()[1::2], map(int, r.stdout.split()[2::2])))


def test_every_state_chooses_the_same_trip(model):
    got = run(model, "choice")
    assert got["bad"] == 0
    # five bounds x the 47 905 triples of at most 64 lanes x the debts a triple can be asked at: at least one each
    assert got["states"] >= 5 * 47905


def test_any_lane_over_masks(model):
    got = run(model, "masks")
    assert got["bad"] == 0 and got["cases"] > 400000


def test_random_sequences_choose_the_same_trips(model):
    got = run(model, "sequence")
    assert got["bad"] == 0
    assert got["leave"] > 1000 and got["pass"] > 1000 and got["step"] > 1000  # (every kind of choice occurs)


def test_a_bound_of_zero_is_refused_where_the_bound_is_made(model):
    got = run(model, "bound")
    assert got["made"] >= 1 and got["runs"] == 1
    assert got["zero_refused"] == 1 and got["zero_valid"] == 0 and got["one_valid"] == 1


def test_the_kernel_compiles_the_header():
    """The kernel asks the header, not copies of its own: the predicates' former text is gone from kernel_wavefront.hip except
    where an instantiation keeps it on purpose (kTripChoice)."""
    with open(os.path.join(CSRC, "kernel_wavefront.hip")) as f:
        text = f.read()
    assert '#include "trip_choice.h"' in text
    for name in ("ptmi_trip::path_logic_due(", "ptmi_trip::pass_is_due<kLeafLanes, kLeafRatio>(", "ptmi_trip::any_lane("):
        assert text.count(name) == 1, name
    with open(os.path.join(CSRC, "kernel_choice.h")) as f:
        assert len(re.findall(r"wait_debt_bound_is_valid\(", f.read())) >= 4  # the three constants and with_instance
