"""Every answer the convolution dispatchers give without launching, over the sweep and the models' layers.

    python tests/golden/make_dispatch_table.py          # rewrites tests/golden/dispatch_table.json

The entry points recorded here are host arithmetic (the view pointers are never dereferenced, bp_conv_pack_job writes
one struct into a host buffer), so the table is the same with and without a GPU.  tests/test_dispatch_table.py
recomputes it and requires equality entry by entry: a refactor of the host code that picks kernels, sizes packed images
or sizes workspaces must leave it as it is; a pull request that changes a kernel choice on purpose re-records it.

Cases: conv_sweep.tagged_cases() at the sweep's own (n, h, w), and the distinct layers of the models
(test_conv_sweep_ref.MODEL_LAYER_IDS) at 512^2 and 64^2 with batch 1 and 64.  The environment switches are read once
into statics, so the whole table is computed once per entry of SETTINGS, each in a child process.

Per case, COLUMNS in order.  Five pairs of views (module input, module output): fp32 aligned ("ff"), fp32 with channel
offset 1 inside a stride of c + 3 ("mis"), and the mixed / bf16 pairs "fb", "bf", "bb".

The file keeps the default setting's rows in full and, for every other setting, only the rows that differ from it.
"""
import ctypes as C
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

PATH = os.path.join(HERE, "dispatch_table.json")

SETTINGS = ("", "BP_FLATW_THIN", "BP_FLATG_THIN", "BP_NOFLAT", "BP_NOSMALL", "BP_NOSTEM", "BP_NOENC")
SWITCHES = tuple(s for s in SETTINGS if s)

VIEW_PAIRS = ("ff", "mis", "fb", "bf", "bb")
_PER_DIR = ("kernel_id", "packed_floats", "bf16_packed_elems", "bf16_supported:null", "pack_job_rc") + tuple(
    "%s:%s" % (q, v) for v in VIEW_PAIRS for q in ("bf16_supported", "ws_kind", "stats_ws:mfma", "stats_ws:bf16"))
COLUMNS = tuple("%s:%s" % (d, q) for d in ("fwd", "bwd") for q in _PER_DIR) + tuple(
    "%s:%s" % (q, v) for v in VIEW_PAIRS for q in ("bwd_data_act_ws", "bwd_weight_ws"))


def cases():
    """[(tag, (transposed, cin, cout, k, stride, pad, out_pad, n, h, w))]"""
    import conv_sweep as S
    from test_conv_sweep_ref import MODEL_LAYER_IDS
    out = list(S.tagged_cases())
    for conv in MODEL_LAYER_IDS:
        for size in (512, 64):
            for n in (1, 64):
                out.append(("model:%s:%d:n%d" % ("_".join(map(str, conv)), size, n), tuple(conv) + (n, size, size)))
    return out


def _views(L, case, pair):
    """(module input view, module output view) of a case; `pair` names (dtype of x, dtype of y) or the odd fp32 view."""
    import conv_sweep as S
    tr, ci, co, k, s, p, op, n, h, w = case
    ho, wo = S.out_shape(case)
    if pair == "mis":
        return (L.View(0x10000, n, h, w, ci, ci + 3, 1, L.F32), L.View(0x20000, n, ho, wo, co, co + 3, 1, L.F32))
    dt = {"f": L.F32, "b": L.BF16}
    return (L.View(0x10000, n, h, w, ci, ci, 0, dt[pair[0]]), L.View(0x20000, n, ho, wo, co, co, 0, dt[pair[1]]))


def row(lib, L, case, job):
    cv = L.Conv(*case[:7])
    pcv = C.byref(cv)
    nblocks = C.c_int64(0)
    out = []
    for d in (L.PACK_FWD, L.PACK_BWD):
        out += [lib.bp_conv_kernel_id(pcv, d), lib.bp_conv_packed_floats(pcv, d), lib.bp_conv_bf16_packed_elems(pcv, d),
                lib.bp_conv_bf16_supported(pcv, d, None, None),
                lib.bp_conv_pack_job(pcv, d, 0x30000, 0x40000, job, C.byref(nblocks))]
        for pair in VIEW_PAIRS:
            x, y = _views(L, case, pair)
            gin, gout = (x, y) if d == L.PACK_FWD else (y, x)
            out += [lib.bp_conv_bf16_supported(pcv, d, C.byref(gin), C.byref(gout)),
                    lib.bp_conv_ws_kind(pcv, d, C.byref(gin), C.byref(gout)),
                    lib.bp_conv_stats_workspace(pcv, d, C.byref(x), C.byref(y), L.IMPL_MFMA),
                    lib.bp_conv_stats_workspace(pcv, d, C.byref(x), C.byref(y), L.IMPL_BF16)]
    for pair in VIEW_PAIRS:
        x, y = _views(L, case, pair)
        out += [lib.bp_conv_backward_data_act_workspace(pcv, C.byref(y), C.byref(x)),
                lib.bp_conv_backward_weight_workspace(pcv, C.byref(x), C.byref(y))]
    assert len(out) == len(COLUMNS)
    return out


def compute():
    """Rows of every case under THIS process's environment."""
    from baryon_painter_amd import _lib as L
    lib = L.load()
    job = C.create_string_buffer(max(int(lib.bp_conv_pack_job_bytes()), 1))
    return [row(lib, L, case, job) for _, case in cases()]


def compute_setting(setting):
    """Rows under `setting` (a switch name, "": none of them), computed in a child process."""
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    if setting:
        env[setting] = "1"
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "--rows"]
    return json.loads(subprocess.run(cmd, env=env, check=True, stdout=subprocess.PIPE).stdout.decode().splitlines()[-1])


def pack(tables):
    """{setting: rows} -> the committed form."""
    base = tables[""]
    return {"columns": list(COLUMNS), "tags": [t for t, _ in cases()], "default": base,
            "settings": {s: {str(i): r for i, (r, b) in enumerate(zip(tables[s], base)) if r != b} for s in SWITCHES}}


def unpack(doc):
    """The committed form -> {setting: rows}."""
    base = doc["default"]
    out = {"": base}
    for s, diff in doc["settings"].items():
        out[s] = [diff.get(str(i), b) for i, b in enumerate(base)]
    return out


def load():
    with open(PATH) as f:
        return json.load(f)


def main():
    if "--rows" in sys.argv:
        print(json.dumps(compute(), separators=(",", ":")))
        return
    doc = pack({s: compute_setting(s) for s in SETTINGS})
    with open(PATH, "w") as f:
        f.write("{\n")
        f.write('"columns": %s,\n' % json.dumps(doc["columns"]))
        f.write('"tags": %s,\n' % json.dumps(doc["tags"]))
        f.write('"default": [\n%s\n],\n' % ",\n".join(json.dumps(r, separators=(",", ":")) for r in doc["default"]))
        f.write('"settings": {\n%s\n}\n}\n' % ",\n".join(
            '"%s": {%s}' % (s, ",".join('\n"%s":%s' % (i, json.dumps(r, separators=(",", ":"))) for i, r in d.items()))
            for s, d in doc["settings"].items()))
    print("%d cases x %d columns x %d settings -> %s (%d bytes)" % (
        len(doc["tags"]), len(COLUMNS), len(SETTINGS), PATH, os.path.getsize(PATH)))


if __name__ == "__main__":
    main()
