"""Every ops.<name>( call of the model is either a predicate / plan / image builder or an entry the launch census records and
checks against float64 (tests/launch_census.py, tests/test_launch_census_gpu.py): a new kernel entry cannot escape the census."""
import os
import re

import launch_census as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = ("acr_wsss_amd/backbone.py", "acr_wsss_amd/DPT/ACR.py", "acr_wsss_amd/infer_cam.py", "acr_wsss_amd/train.py")
CALL = re.compile(r"(?<![\w.])_?ops\.([A-Za-z_]\w*)\s*\(")


def called_names(text):
    return set(CALL.findall(text))


def uncovered(names):
    return sorted(n for n in names if not LC.is_not_a_launch(n) and n not in LC.CHECKERS)


def test_every_ops_call_of_the_model_is_censused_or_a_predicate():
    found = {}
    for rel in SOURCES:
        with open(os.path.join(ROOT, rel)) as f:
            for n in called_names(f.read()):
                found.setdefault(n, []).append(rel)
    assert len(found) >= 20, sorted(found)                  # the scan sees the model's calls (not an empty match)
    missing = uncovered(found)
    assert not missing, "ops entries the model calls with no census checker: %s" % {n: found[n] for n in missing}


def test_census_entries_and_checkers_agree():
    from acr_wsss_amd import ops
    assert set(LC.CHECKERS) == set(LC.ENTRIES)
    for n in LC.ENTRIES:
        assert callable(getattr(ops, n)), n
    for n in LC.NOT_LAUNCHES:
        assert hasattr(ops, n), n


def test_the_scan_catches_a_new_entry():
    src = "x = ops.conv3x3(x, w)\ny = _ops.consistency(a, p)\nif ops.conv3x3_fusable(x):\n    z = ops.foo_new_kernel(x)\n"
    names = called_names(src)
    assert names == {"conv3x3", "consistency", "conv3x3_fusable", "foo_new_kernel"}
    assert uncovered(names) == ["foo_new_kernel"]
