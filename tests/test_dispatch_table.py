"""CPU: every answer the convolution dispatchers give without launching equals tests/golden/dispatch_table.json.

The table (tests/golden/make_dispatch_table.py) holds kernel ids, packed-image sizes, bf16 support, the
weights-stationary kind and every workspace size of the sweep's cases and the models' layers, once per environment
switch that moves a layer between kernel families.  The host code that answers them is a table of kernel families walked
in priority order; the six things asked of a layer (is it yours, id, image size, pack, workspace, run) must come from the
same family, and this is where a disagreement shows without a GPU.
"""
from concurrent.futures import ThreadPoolExecutor

from golden import make_dispatch_table as M


def test_dispatch_answers_equal_the_recorded_table():
    doc = M.load()
    tagged = M.cases()
    assert doc["columns"] == list(M.COLUMNS) and doc["tags"] == [t for t, _ in tagged]
    assert set(doc["settings"]) == set(M.SWITCHES)
    want = M.unpack(doc)
    # (the switches are read once into statics: one child process per setting, all at once)
    with ThreadPoolExecutor(max_workers=len(M.SETTINGS)) as ex:
        got = dict(zip(M.SETTINGS, ex.map(M.compute_setting, M.SETTINGS)))
    wrong = []
    for s in M.SETTINGS:
        assert len(got[s]) == len(want[s]) == len(tagged)
        for (tag, case), g, w in zip(tagged, got[s], want[s]):
            wrong += ["%s %s %s [%s]: got %d, recorded %d" % (tag, case, col, s or "default", a, b)
                      for col, a, b in zip(M.COLUMNS, g, w) if a != b]
    print("\n%d settings x %d cases x %d columns compared" % (len(M.SETTINGS), len(tagged), len(M.COLUMNS)))
    assert not wrong, "%d entries differ:\n%s" % (len(wrong), "\n".join(wrong[:40]))
    # BP_FLATW_THIN is the one setting under which two families (flat_t64 and flat_t4) accept the same layer
    # ... and flat_t64 takes it: its id and the size of its image (cin * cout * 16), not flat_t4's 720000
    i = doc["tags"].index("gate:flat_t4_32_16")
    col = {c: j for j, c in enumerate(M.COLUMNS)}
    for table in (got, want):
        assert table[""][i][col["fwd:kernel_id"]] == 720000
        assert table["BP_FLATW_THIN"][i][col["fwd:kernel_id"]] == 740000
        assert table["BP_FLATW_THIN"][i][col["fwd:packed_floats"]] == 32 * 16 * 16
