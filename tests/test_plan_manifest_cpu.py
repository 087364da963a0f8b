"""Every known plan lowers as on the commit that recorded tests/golden/plan_manifest.json: the same
describe() text, kernel list (names, flops, bytes), weight and workspace bytes, for every case and
arm of tools/plan_manifest.py.  No GPU: plans are declared, never finalized.  A mismatch is
diagnosed with `tools/plan_manifest.py --dump CASE` on the two checkouts."""
import importlib.util
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def _tool():
    spec = importlib.util.spec_from_file_location("plan_manifest", os.path.join(os.path.dirname(HERE), "tools",
                                                                                 "plan_manifest.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_case_lowers_as_recorded():
    pm = _tool()
    want, got = pm.load(), pm.compute()
    assert len(want) >= 190 and len(pm.ARMS) == 45
    # the fixture is not vacuous: every case declares as a batch-64 fp32 plan with at least one kernel
    assert all(r["b64"] != "error" and r["b64"][2] >= 1 and len(r["sha256"]) == 64 for r in want.values())
    bad = pm.differences(want, got)
    assert not bad, "%d cases differ, the first:\n%s" % (len(bad), "\n".join(bad[:10]))
