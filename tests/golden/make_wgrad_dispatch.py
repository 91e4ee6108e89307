"""bp_conv_backward_weight_plan and the workspace query over the sweep and the models' layers, once per switch.

    python tests/golden/make_wgrad_dispatch.py          # rewrites tests/golden/wgrad_dispatch.json

make_wgrad_plan.py records the queries over the cases of tests/wgrad_sweep.py, which are picked per kernel; this table
asks the same QUERIES of every case of make_dispatch_table.cases() -- the conv sweep and the distinct model layers at
512^2 and 64^2 with batch 1 and 64 -- so that it holds what the weight-gradient dispatcher answers wherever a layer can
land: [return code, family, nsplit, cxp, cyp, bp_conv_backward_weight_workspace] per (case, query).  The answers are
host arithmetic, the same with and without a GPU.  tests/test_wgrad_sweep_host.py recomputes the table and requires
equality entry by entry: a refactor of the host code that picks the kernels or sizes their workspaces must leave it as
it is; a pull request that changes a choice on purpose re-records it.

The environment switches are read once into statics, so the whole table is computed once per entry of SETTINGS, each in
a child process.  The numeric tuning variables (BP_WT_TARGET and the like) are left out.

The file: "rows" lists every distinct answer once (the models' layers repeat most of them); "default" holds, per case in
the order of cases(), the indices into "rows" of its answers to QUERIES; "settings" holds the same for every other
setting, only for the cases (by index) whose answers differ from the default's.  The cases' tags are those of
tests/golden/dispatch_table.json.
"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from golden import make_dispatch_table as D  # noqa: E402
from golden import make_wgrad_plan as M  # noqa: E402

PATH = os.path.join(HERE, "wgrad_dispatch.json")

# every switch that moves a weight-gradient layer between families ("NAME" sets NAME=1)
SETTINGS = ("", "BP_NOSTEM", "BP_NOENC", "BP_NOTHIN", "BP_NOWFLAT", "BP_NOWFLAT_S2", "BP_WT_NODMA", "BP_F32_WGRAD_WS=0",
            "BP_BF16_WGRAD_WS=0", "BP_BF16_NOFLATW", "BP_BF16_NOHEADW", "BP_BF16_NOWT")
SWITCHES = tuple(s for s in SETTINGS if s)
QUERIES = M.QUERIES
cases = D.cases


def compute():
    """Rows of every case under THIS process's environment."""
    from baryon_painter_amd import _lib as L
    lib = L.load()
    return [[M.plan(lib, L, case, impl, kind, dt) for _, impl, kind, dt in QUERIES] for _, case in cases()]


def compute_setting(setting):
    """Rows under `setting` ("": none of the switches), computed in a child process."""
    names = {s.split("=")[0] for s in SWITCHES}
    env = {k: v for k, v in os.environ.items() if k not in names}
    if setting:
        name, _, value = setting.partition("=")
        env[name] = value or "1"
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "--rows"]
    return json.loads(subprocess.run(cmd, env=env, check=True, stdout=subprocess.PIPE).stdout.decode().splitlines()[-1])


def pack(tables):
    """{setting: rows} -> the committed form."""
    index = {}
    ids = lambda case_rows: [index.setdefault(tuple(r), len(index)) for r in case_rows]
    base = tables[""]
    doc = {"queries": [q[0] for q in QUERIES], "default": [ids(r) for r in base],
           "settings": {s: {str(i): ids(r) for i, (r, b) in enumerate(zip(tables[s], base)) if r != b} for s in SWITCHES}}
    doc["rows"] = [list(r) for r in index]
    return doc


def unpack(doc):
    """The committed form -> {setting: rows}."""
    rows = lambda ids: [doc["rows"][i] for i in ids]
    base = [rows(ids) for ids in doc["default"]]
    out = {"": base}
    for s, diff in doc["settings"].items():
        out[s] = [rows(diff[str(i)]) if str(i) in diff else b for i, b in enumerate(base)]
    return out


def _lines(items, per_line):
    """JSON of a list, `per_line` items per line."""
    items = [json.dumps(v, separators=(",", ":")) for v in items]
    return ",\n".join(",".join(items[i:i + per_line]) for i in range(0, len(items), per_line))


def write(doc):
    with open(PATH, "w") as f:
        f.write("{\n")
        f.write('"queries": %s,\n' % json.dumps(doc["queries"]))
        f.write('"rows": [\n%s\n],\n' % _lines(doc["rows"], 6))
        f.write('"default": [\n%s\n],\n' % _lines(doc["default"], 4))
        f.write('"settings": {\n%s\n}\n}\n' % ",\n".join(
            '"%s": {\n%s\n}' % (s, ",\n".join('"%s":%s' % (i, json.dumps(r, separators=(",", ":"))) for i, r in d.items()))
            for s, d in doc["settings"].items()))


def load():
    with open(PATH) as f:
        return json.load(f)


def main():
    if "--rows" in sys.argv:
        print(json.dumps(compute(), separators=(",", ":")))
        return
    doc = pack({s: compute_setting(s) for s in SETTINGS})
    write(doc)
    print("%d cases x %d queries x %d settings, %d distinct rows -> %s (%d bytes)" % (
        len(doc["default"]), len(QUERIES), len(SETTINGS), len(doc["rows"]), PATH, os.path.getsize(PATH)))


if __name__ == "__main__":
    main()
