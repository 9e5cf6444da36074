"""The package's public surface against tests/golden/python_api_surface.json, the record taken at the commit before the
bindings moved onto binding.py (tests/golden/make_python_api_surface.py says what it holds).  The surface is regenerated
in memory and must equal the record, but for the differences listed here, each one an addition or an annotation."""
import copy
import importlib.util
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_python_api_surface", os.path.join(HERE, "golden", "make_python_api_surface.py"))
_gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_gen)

NEW_MODULES = {"binding"}
# the kinds are defined once, in ivf_ann; shard_set and faiss_files go on exporting them
ADDED_CONSTANTS = {"ivf_ann": {"KIND_IVF_FLAT": 1, "KIND_IVF_PQ": 2, "KIND_OPQ_IVF_PQ": 3}}
# close() is Handle's, annotated `-> None`; these two were written without the annotation
CLOSE_GAINED_ANNOTATION = [("hnsw_ann", "Hnsw"), ("ann_by_id", "Hnsw"), ("representation_scorer", "EmbeddingStore")]
# ann_codec has no `from __future__ import annotations`; its _check comes from binding.py, which has
CHECK_ANNOTATIONS_AS_STRINGS = ("ann_codec", "(lib, rc: int) -> None", "(lib, rc: 'int') -> 'None'")


def test_surface_is_the_recorded_one(pkg):
    with open(os.path.join(HERE, "golden", "python_api_surface.json")) as f:
        recorded = json.load(f)
    now = json.loads(_gen.dumps(_gen.surface()))
    assert set(now) - set(recorded) == NEW_MODULES and not set(recorded) - set(now)
    expected = copy.deepcopy(recorded)
    for module, constants in ADDED_CONSTANTS.items():
        expected[module]["constants"].update(constants)
        expected[module]["names"] = sorted(expected[module]["names"] + list(constants))
    for module, cls in CLOSE_GAINED_ANNOTATION:
        members = expected[module]["classes"][cls]["members"]
        assert members["close"] == "(self)"
        members["close"] = "(self) -> 'None'"
    module, before, after = CHECK_ANNOTATIONS_AS_STRINGS
    assert expected[module]["functions"]["_check"] == before
    expected[module]["functions"]["_check"] = after
    for module in recorded:
        for part in recorded[module]:
            assert now[module][part] == expected[module][part], (module, part)
