"""Round 12's host-side pieces, no GPU: which gather offsets the two-wave units get, and the listing parser of
tools/unit_kernel_issue_budget.py."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def budget():
    spec = importlib.util.spec_from_file_location("unit_kernel_issue_budget", os.path.join(ROOT, "tools", "unit_kernel_issue_budget.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_offsets_are_narrow_below_two_to_the_29_postings(pkg):
    """8-byte positions fit a 32-bit byte offset while 8 * n_postings < 2^32; sann_unit_offset_bits is the function
    sann_batch_prepare decides with (FastParams::wide_offsets)."""
    f = pkg.load_library().sann_unit_offset_bits
    assert f(0, 0) == 32 and f(1, 0) == 32
    assert f((1 << 29) - 1, 0) == 32
    assert f(1 << 29, 0) == 64
    assert f((1 << 32) - 1, 0) == 64 and f(1 << 40, 0) == 64
    # SANN_UNIT_OFFSETS=64 forces the wide form, never the narrow one
    assert f((1 << 29) - 1, 1) == 64 and f(1, 1) == 64 and f(1 << 29, 1) == 64


def test_mangled_template_arguments(budget):
    assert budget.mangled_args("128,12,64,0,false,true") == "ILi128ELi12ELi64ELi0ELb0ELb1EE"
    assert budget.mangled_args("128, 12, 64, 0, false, true, true") == "ILi128ELi12ELi64ELi0ELb0ELb1ELb1EE"


def test_listing_parser_counts_per_region(budget):
    text = open(os.path.join(ROOT, "tests", "golden", "unit_issue_listing.txt")).read()
    regions = budget.parse_listing(text, args="128,12,64,0,false,true,false")
    assert regions == [
        dict(vector=1, mul=0, cmp64=0, scalar=3, lds=1, **{"global": 0}),   # (the barrier counts in the region it ends)
        dict(vector=9, mul=3, cmp64=2, scalar=5, lds=2, **{"global": 1}),   # (v_mul_f32 is no integer multiply; s_waitcnt in the asm block counts)
        dict(vector=1, mul=0, cmp64=1, scalar=1, lds=0, **{"global": 4}),   # (stops at the function's end label)
    ]
    assert budget.totals(regions) == dict(vector=11, mul=3, cmp64=3, scalar=9, lds=3, **{"global": 5})
    # the other instantiation of the file is found by its own arguments; one that is not there is an error
    assert budget.parse_listing(text, args="256,6,64,0,false,true,false") == [
        dict(vector=1, mul=1, cmp64=0, scalar=1, lds=0, **{"global": 0}), dict(vector=0, mul=0, cmp64=0, scalar=1, lds=0, **{"global": 0})]
    with pytest.raises(LookupError):
        budget.parse_listing(text, args="128,12,64,0,false,true")


def test_classification_is_by_prefix_and_a_few_names(budget):
    c = budget.classify
    assert c("v_mad_u64_u32") == ["vector", "mul"] and c("v_mul_lo_u32") == ["vector", "mul"] and c("v_mul_hi_u32_e64") == ["vector", "mul"]
    assert c("v_mul_f64") == ["vector"] and c("v_lshl_add_u64") == ["vector"]
    assert c("v_cmp_ne_u64_e32") == ["vector", "cmp64"] and c("v_cmpx_le_i64_e64") == ["vector", "cmp64"] and c("v_cmp_lt_i32_e32") == ["vector"]
    assert c("s_and_saveexec_b64") == ["scalar"] and c("ds_or_rtn_b64") == ["lds"] and c("global_load_dwordx2") == ["global"]
    assert c(".p2align") == [] and c("image_load") == []
