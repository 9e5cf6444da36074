"""Round 13's host-side pieces, no GPU: tools/unit_kernel_issue_budget.py pointed at other kernels than the unit kernel
(--kernel, --source), on an excerpt of this build's own listings, and the refusal of the 128-bit wave-sort hook."""
import importlib.util
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "unit_kernel_issue_budget.py")
LISTING = os.path.join(ROOT, "tests", "golden", "merge_issue_listing.txt")


@pytest.fixture(scope="module")
def budget():
    spec = importlib.util.spec_from_file_location("unit_kernel_issue_budget_r13", TOOL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _row(vector, mul, cmp64, scalar, lds, glob):
    return dict(vector=vector, mul=mul, cmp64=cmp64, scalar=scalar, lds=lds, **{"global": glob})


def test_parser_finds_other_kernels_by_name_and_arguments(budget):
    text = open(LISTING).read()
    # merge_kernel<512, 1728>: the head up to its second barrier (the excerpt ends right behind it: an empty last region)
    assert budget.parse_listing(text, kernel="merge_kernel", args="512,1728") == [
        _row(31, 0, 0, 86, 1, 3), _row(61, 5, 0, 55, 6, 0), _row(0, 0, 0, 0, 0, 0)]
    # one wave per query: no barrier, one region
    assert budget.parse_listing(text, kernel="merge_wave_kernel", args="4,8") == [_row(36, 0, 0, 34, 0, 10)]
    assert budget.parse_listing(text, kernel="desc_query_kernel", args="1") == [_row(20, 0, 0, 55, 2, 3)]
    # "merge_kernel" is no prefix match of merge_wave_kernel's symbol, and the arguments are part of the name
    with pytest.raises(LookupError):
        budget.parse_listing(text, kernel="merge_kernel", args="4,8")
    with pytest.raises(LookupError):
        budget.parse_listing(text, kernel="merge_wave_kernel", args="8,16")
    with pytest.raises(LookupError):
        budget.parse_listing(text, args="512,1728")  # the default kernel is the unit kernel


def test_defaults_are_the_unit_kernel_of_sann_fast(budget):
    assert budget.DEFAULT_KERNEL == "unit_fast_kernel" and budget.DEFAULT_SOURCE == "sann_fast.hip"
    assert budget.DEFAULT_ARGS == "128,12,64,0,false,true"


def test_command_line_reports_the_named_kernel():
    run = lambda *a: subprocess.run([sys.executable, TOOL, "--listing", LISTING] + list(a), capture_output=True, text=True)
    r = run("--kernel", "merge_kernel", "--args", "512,1728")
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert lines[0].startswith("merge_kernel<512,1728>: instructions per region")
    assert lines[-1].split() == ["total", "92", "5", "0", "141", "7", "3"]
    r = run("--kernel", "merge_wave_kernel", "--args", "4,8", "--source", "sann_kernels.hip")  # (--listing: nothing is compiled)
    assert r.returncode == 0 and r.stdout.splitlines()[-1].split() == ["total", "36", "0", "0", "34", "0", "10"]
    r = run("--kernel", "merge_kernel", "--args", "512,1728", "--compare", LISTING, LISTING)
    assert r.returncode == 0 and r.stdout.splitlines()[-1].split() == ["delta", "+0", "+0", "+0", "+0", "+0", "+0"]
    assert run().returncode != 0  # the excerpt holds no unit kernel


def test_k128_sort_hook_refuses_a_null_array_before_any_device_call(pkg):
    """A negative count asks for the 128-bit network; without an array it is SANN_EINVAL, on a machine without a device too."""
    lib = pkg.load_library()
    assert lib.sann_debug_wave_sort(0, -1, None) == 1
    assert b"bad arguments" in lib.sann_last_error()
    assert lib.sann_debug_wave_sort(0, -(2 ** 31), None) == 1
    assert lib.sann_debug_wave_sort(0, 1, None) == 1
    assert lib.sann_debug_wave_sort(0, 0, None) == 0  # nothing to sort
