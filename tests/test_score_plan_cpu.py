"""The score network's launch plan (arreau_amd/csrc/score_plan.h) against a table written out by hand from its rules: every
threshold on the batch size, the model and the switches.  tests/score_plan_host.cpp is compiled with the host C++ compiler -- no
HIP, no device -- and run once for all rows.

Defaults of a row: the flagship model (fused, C 128, D 256, H 512, L 2, k 8, S 90, weights inside fp16, both fp8 formats calibrated
in), edge / mlp / conv / read-out variants 4 / 3 / 2 / 1, 256 CUs, every switch unset, N = 100.  A row overrides what it names and
states what it expects of the plan; codes = edge / mlp / conv / read-out kernel, basis row bytes, fp8 cross products as
arreau_model_status reports them."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

# what a launch of at most 240 atoms on the default model runs: split edge kernel, one-launch small layer, split MFMA read-out
SMALL = dict(general=0, edge="f16x3", form="split", wgs=0, basis_form=0, basis_fp8=1, cross_fp8=1, message="small_layer", boustrophedon=1,
             mlp="small_layer", nb=0, slots=0, readout="mfma_split", no_prep=1, codes="4/3/1/1/0/0")
# a large launch: basis form
LARGE = dict(general=0, edge="f16x3", form="persistent", wgs=256, basis_form=1, basis_fp8=1, cross_fp8=1, message="basis_proj",
             boustrophedon=1, mlp="f16x3_tile", slots=3, no_prep=1)
GENERAL = dict(general=1, edge="none", form="persistent", wgs=0, basis_form=0, basis_fp8=0, cross_fp8=0, message="register", boustrophedon=0,
               mlp="fp32", nb=0, slots=0, readout="vector", no_prep=0, codes="5/5/5/5/0/0")

ROWS = [
    # ---- N: the edge kernel's split form (<= 240), the basis form (> 2000), the small layer and the split ConvNext form (<= 512)
    ("N=240", SMALL),
    ("N=241", {**SMALL, "form": "persistent", "wgs": 121}),
    ("N=512", {**SMALL, "form": "persistent", "wgs": 256}),
    ("N=513", dict(message="streamed", mlp="f16x3_tile", nb=1, slots=3, basis_form=0, codes="4/3/1/1/0/0")),
    ("N=2000", dict(basis_form=0, form="persistent", wgs=256, message="streamed", mlp="f16x3_tile", nb=1, readout="mfma_split",
                    codes="4/3/1/1/0/0")),
    ("N=2001", {**LARGE, "nb": 1, "readout": "mfma_split", "codes": "4/3/2/1/768/1"}),
    # ARREAU_BASIS_MIN_RECEIVERS moves the switch, never below 240
    ("N=240 BASIS_MIN_RECEIVERS=240", SMALL),
    ("N=241 BASIS_MIN_RECEIVERS=240", dict(basis_form=1, form="persistent", wgs=121, message="basis_proj", mlp="f16x3_split", nb=0, slots=0,
                                           codes="4/3/2/1/768/1")),
    ("N=2000 BASIS_MIN_RECEIVERS=240", dict(basis_form=1, mlp="f16x3_tile")),
    ("N=2001 BASIS_MIN_RECEIVERS=240", dict(basis_form=1)),
    ("N=240 BASIS_MIN_RECEIVERS=0", SMALL),
    ("N=241 BASIS_MIN_RECEIVERS=0", dict(basis_form=1, message="basis_proj", mlp="f16x3_split")),
    ("N=2000 BASIS_MIN_RECEIVERS=0", dict(basis_form=1)),
    ("N=2001 BASIS_MIN_RECEIVERS=0", dict(basis_form=1)),
    ("N=240 BASIS_MIN_RECEIVERS=5000", SMALL),
    ("N=241 BASIS_MIN_RECEIVERS=5000", dict(basis_form=0, message="small_layer")),
    ("N=2000 BASIS_MIN_RECEIVERS=5000", dict(basis_form=0)),
    ("N=2001 BASIS_MIN_RECEIVERS=5000", dict(basis_form=0, message="streamed", codes="4/3/1/1/0/0")),
    ("N=5000 BASIS_MIN_RECEIVERS=5000", dict(basis_form=0)),
    ("N=5001 BASIS_MIN_RECEIVERS=5000", dict(basis_form=1)),
    # the calibration: basis form from 241 atoms whatever the switches say, formats from the model's fields alone
    ("N=241 calibrating=1", dict(basis_form=1, message="basis_proj", mlp="f16x3_split", codes="4/3/2/1/768/1")),
    ("N=240 calibrating=1", dict(basis_form=0)),
    ("N=320 calibrating=1 BASIS_MIN_RECEIVERS=5000 BASIS_FP8=0 CROSS_FP8=0", dict(basis_form=1, basis_fp8=1, cross_fp8=1)),
    ("N=320 calibrating=1 BASIS_FP8=1 fp8_ok=0 x8_ok=0", dict(basis_form=1, basis_fp8=0, cross_fp8=0, codes="4/3/2/1/1024/0")),
    ("N=320 calibrating=1 fp8_ok=1 x8_ok=0", dict(basis_fp8=1, cross_fp8=0, codes="4/3/2/1/768/0")),
    # the read-out splits while ceil(N / 32) < 256
    ("N=8160", {**LARGE, "readout": "mfma_split"}),
    ("N=8161", {**LARGE, "readout": "mfma", "codes": "4/3/2/1/768/1"}),
    # nodes per wave of the tile form: 1 when 6 ceil(N / 2048) < 10 ceil(ceil(N / 2) / 2048)
    ("N=2048", dict(mlp="f16x3_tile", nb=1)),   # 6 * 1 < 10 * 1
    ("N=2049", dict(mlp="f16x3_tile", nb=2)),   # 6 * 2 > 10 * 1
    ("N=4096", dict(mlp="f16x3_tile", nb=2)),   # 6 * 2 > 10 * 1
    ("N=4097", dict(mlp="f16x3_tile", nb=1)),   # 6 * 3 < 10 * 2
    ("N=6144", dict(mlp="f16x3_tile", nb=1)),   # 6 * 3 < 10 * 2
    ("N=6145", dict(mlp="f16x3_tile", nb=2)),   # 6 * 4 > 10 * 2
    ("N=2048 n_cu=128", dict(nb=2)),             # 1024 slots: 6 * 2 > 10 * 1
    # ---- the model
    ("L=1", {**SMALL, "form": "persistent", "wgs": 50}),
    ("L=2", SMALL),
    ("L=6", SMALL),
    ("L=7", {**SMALL, "form": "persistent", "wgs": 50}),
    ("L=8", {**SMALL, "form": "persistent", "wgs": 50}),
    ("L=9", {**SMALL, "form": "persistent", "wgs": 50, "readout": "vector", "codes": "4/3/1/0/0/0"}),
    ("L=1 N=3000", dict(basis_form=0, message="streamed")),
    ("L=2 N=3000", dict(basis_form=1)),
    ("L=8 N=9000", dict(basis_form=1, readout="mfma")),
    ("L=9 N=9000", dict(basis_form=1, readout="vector")),
    ("k=8", SMALL),
    ("k=6", {**SMALL, "message": "register", "mlp": "f16x3_split", "codes": "4/3/0/1/0/0"}),
    ("k=6 N=3000", dict(basis_form=0, message="register", mlp="f16x3_tile", codes="4/3/0/1/0/0")),
    ("k=8 N=3000", dict(basis_form=1, message="basis_proj")),
    ("f16_ok=0", dict(edge="bf16x6", form="persistent", wgs=0, basis_form=0, message="streamed", mlp="bf16x6", codes="3/1/1/1/0/0")),
    ("f16_ok=0 N=3000", dict(edge="bf16x6", basis_form=0, message="streamed", mlp="bf16x6", nb=0, codes="3/1/1/1/0/0")),
    ("f16_ok=1 N=3000", dict(edge="f16x3", basis_form=1, mlp="f16x3_tile", codes="4/3/2/1/768/1")),
    ("x8_ok=0 N=3000", dict(basis_fp8=1, cross_fp8=0, codes="4/3/2/1/768/0")),
    ("x8_ok=1 N=3000", dict(basis_fp8=1, cross_fp8=1, codes="4/3/2/1/768/1")),
    ("fp8_ok=0 N=3000", dict(basis_fp8=0, cross_fp8=0, codes="4/3/2/1/1024/0")),
    ("fp8_ok=0", {**SMALL, "basis_fp8": 0, "cross_fp8": 0}),
    ("S=92", dict(readout="mfma_split")),             # S + 4 = 96
    ("S=93", dict(readout="vector", codes="4/3/1/0/0/0")),  # 97
    ("S=93 N=9000", dict(readout="vector")),
    ("C=64", dict(basis_form=0, mlp="f16x3_split", readout="vector")),   # (a fused model has C 128: the rules ask all the same)
    ("H=256", dict(mlp="f16x3_split", message="streamed")),
    ("D=128 N=3000", dict(basis_form=0)),
    # ---- conv and read-out variants
    ("conv_variant=0", dict(message="register", mlp="f16x3_split", codes="4/3/0/1/0/0")),
    ("conv_variant=1", SMALL),
    ("conv_variant=2", SMALL),
    ("conv_variant=0 N=3000", dict(basis_form=0, message="register", codes="4/3/0/1/0/0")),
    ("conv_variant=1 N=3000", dict(basis_form=0, message="streamed", codes="4/3/1/1/0/0")),
    ("conv_variant=2 N=3000", dict(basis_form=1, message="basis_proj", codes="4/3/2/1/768/1")),
    ("readout_variant=0", dict(readout="vector", codes="4/3/1/0/0/0")),
    ("readout_variant=1", dict(readout="mfma_split", codes="4/3/1/1/0/0")),
    ("readout_variant=0 N=9000", dict(readout="vector")),
    ("readout_variant=1 N=9000", dict(readout="mfma")),
    # ---- each switch forced both ways
    ("BASIS_FP8=0", {**SMALL, "basis_fp8": 0, "cross_fp8": 0}),
    ("BASIS_FP8=1 fp8_ok=0", SMALL),
    ("BASIS_FP8=0 N=3000", dict(basis_fp8=0, cross_fp8=0, codes="4/3/2/1/1024/0")),
    ("BASIS_FP8=1 fp8_ok=0 N=3000", dict(basis_fp8=1, cross_fp8=1, codes="4/3/2/1/768/1")),
    ("CROSS_FP8=0 N=3000", dict(basis_fp8=1, cross_fp8=0, codes="4/3/2/1/768/0")),
    ("CROSS_FP8=1 N=3000", dict(basis_fp8=1, cross_fp8=1)),
    ("CROSS_FP8=1 x8_ok=0 N=3000", dict(cross_fp8=0)),
    ("EDGE_SPLIT=0", {**SMALL, "form": "persistent", "wgs": 50}),
    ("EDGE_SPLIT=1 N=1000", dict(form="split", wgs=0)),
    ("EDGE_SPLIT=1 N=3000", dict(basis_form=1, form="persistent", wgs=256)),   # never with the basis form
    ("EDGE_SPLIT=1 L=7", dict(form="persistent")),                              # nor beyond six layers
    ("EDGE_SPLIT=1 edge_variant=3", dict(edge="bf16x6", form="persistent", wgs=0)),
    ("EDGE_WGS=64 N=1000", dict(form="persistent", wgs=64)),
    ("EDGE_WGS=1000 N=300", dict(form="persistent", wgs=150)),
    ("EDGE_WGS=0 N=1000", dict(form="persistent", wgs=256)),
    ("EDGE_WGS=-3 N=1000", dict(wgs=256)),
    ("n_cu=304 N=1000", dict(wgs=304)),
    ("FUSE_SMALL=0", {**SMALL, "message": "streamed", "mlp": "f16x3_split"}),
    ("FUSE_SMALL=1", SMALL),
    ("FUSE_SMALL=0 N=513", dict(mlp="f16x3_tile")),
    ("MLP_SPLIT=1", {**SMALL, "message": "streamed", "mlp": "f16x3_split"}),   # set either way: no small layer
    ("MLP_SPLIT=0", {**SMALL, "message": "streamed", "mlp": "f16x3_tile", "nb": 1, "slots": 3}),
    ("MLP_SPLIT=1 N=3000", dict(mlp="f16x3_split", nb=0, slots=0)),
    ("MLP_SPLIT=0 mlp_variant=4", dict(mlp="f16x3_split", message="streamed")),  # variant 4 is always the split form
    ("mlp_variant=4 N=3000", dict(mlp="f16x3_split")),
    ("mlp_variant=4", dict(mlp="f16x3_split", message="streamed", codes="4/3/1/1/0/0")),
    ("MLP_NB=1 N=2049", dict(nb=1)),
    ("MLP_NB=2 N=2048", dict(nb=2)),
    ("MLP_NB=3 N=2048", dict(nb=1)),
    ("MLP_SLOTS=4 N=3000", dict(mlp="f16x3_tile", slots=4)),
    ("MLP_SLOTS=3 N=3000", dict(slots=3)),
    ("MLP_SLOTS=5 N=3000", dict(slots=3)),
    ("MLP_SLOTS=4", SMALL),
    ("READOUT_SPLIT=0", {**SMALL, "readout": "mfma"}),
    ("READOUT_SPLIT=1 N=9000", dict(readout="mfma_split", codes="4/3/2/1/768/1")),
    ("READOUT_SPLIT=1 S=93", dict(readout="vector")),
    ("CONV_PROJ_BOUSTROPHEDON=0 N=3000", dict(boustrophedon=0, basis_form=1)),
    ("CONV_PROJ_BOUSTROPHEDON=1 N=3000", dict(boustrophedon=1)),
    ("LOOP_PREP=1", {**SMALL, "no_prep": 0}),
    ("LOOP_PREP=0", SMALL),
    # ---- the general network: a shape without fused kernels, or edge variant 5
    ("fused=0 C=12 D=20 H=36 L=3 k=3 S=13", GENERAL),
    ("fused=0 C=12 D=20 H=36 L=3 k=3 S=13 N=3000 LOOP_PREP=0", GENERAL),
    ("edge_variant=5", GENERAL),
    ("edge_variant=5 N=3000 BASIS_MIN_RECEIVERS=240", GENERAL),
    ("none", {**GENERAL, "general": 0, "codes": "-1/-1/-1/-1/0/0"}),
]

# every edge variant against every ConvNext variant, at a size without the small forms (1,000 atoms: K pair, tile form)
EDGE_OF_VARIANT = [("fp32", 0), ("fp32", 0), ("fp32", 0), ("bf16x6", 3), ("f16x3", 4), None]
MLP_OF_VARIANT = [("fp32", 0), ("bf16x6", 1), ("bf16x6", 1), ("f16x3_tile", 3), ("f16x3_split", 3)]
for ev in range(6):
    for mv in range(5):
        row = "N=1000 edge_variant=%d mlp_variant=%d" % (ev, mv)
        if EDGE_OF_VARIANT[ev] is None:
            ROWS.append((row, GENERAL))
            continue
        (edge, edge_code), (mlp, mlp_code) = EDGE_OF_VARIANT[ev], MLP_OF_VARIANT[mv]
        ROWS.append((row, dict(general=0, edge=edge, mlp=mlp, basis_form=0, message="streamed", wgs=256 if ev == 4 else 0,
                               nb=1 if mv == 3 else 0, codes="%d/%d/1/1/0/0" % (edge_code, mlp_code))))
# the basis form needs the fp16x3 edge kernel, not the fp16x3 ConvNext kernel
ROWS += [("N=3000 edge_variant=3", dict(basis_form=0, edge="bf16x6", message="streamed", codes="3/3/1/1/0/0")),
         ("N=3000 mlp_variant=1", dict(basis_form=1, mlp="bf16x6", codes="4/1/2/1/768/1")),
         ("N=3000 mlp_variant=0", dict(basis_form=1, mlp="fp32", codes="4/0/2/1/768/1")),
         # the small layer does not depend on the edge kernel
         ("edge_variant=0", {**SMALL, "edge": "fp32", "form": "persistent", "codes": "0/3/1/1/0/0"}),
         ("mlp_variant=1", {**SMALL, "message": "streamed", "mlp": "bf16x6", "codes": "4/1/1/1/0/0"})]

# plans that differ in one switch or one input compare unequal, equal rows equal: (row, row before it, equal)
PAIRS = [("N=3000", "N=3000", 1), ("N=3000", "N=3000 CONV_PROJ_BOUSTROPHEDON=0", 0), ("N=3000", "N=3000 CROSS_FP8=0", 0),
         ("N=3000", "N=3000 MLP_SLOTS=4", 0), ("N=3000", "N=3000 LOOP_PREP=1", 0), ("N=3000", "N=3000 READOUT_SPLIT=0", 0),
         ("N=100", "N=100 FUSE_SMALL=0", 0), ("N=100", "N=100 EDGE_SPLIT=0", 0), ("N=100", "N=100 BASIS_FP8=0", 0),
         ("N=1000", "N=1000 EDGE_WGS=64", 0), ("N=1000", "N=1000 readout_variant=0", 0), ("N=3000", "N=3001", 1),
         ("N=2000", "N=2001", 0), ("edge_variant=5", "fused=0", 1), ("none", "edge_variant=5", 0), ("none", "none", 1)]


def _host_compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = name and shutil.which(name)
        if path:
            return path
    pytest.fail("no host C++ compiler found (set CXX)")


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """{row: {field: value}} of every row of ROWS and PAIRS, from one run of the host program."""
    exe = str(tmp_path_factory.mktemp("score_plan") / "score_plan_host")
    subprocess.run([_host_compiler(), "-std=c++20", "-O1", "-Wall", os.path.join(HERE, "score_plan_host.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    rows = [r for r, _ in ROWS] + [r for a, b, _ in PAIRS for r in (b, a)]
    out = subprocess.run([exe], input="\n".join(rows) + "\n", check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(rows)
    parsed = [dict(tok.split("=", 1) for tok in line.split()) for line in out]
    return parsed[:len(ROWS)], parsed[len(ROWS):]


@pytest.mark.parametrize("index", range(len(ROWS)), ids=[r.replace(" ", ",") for r, _ in ROWS])
def test_plan_row(plans, index):
    row, expected = ROWS[index]
    got = plans[0][index]
    assert {k: got[k] for k in expected} == {k: str(v) for k, v in expected.items()}, row


@pytest.mark.parametrize("index", range(len(PAIRS)), ids=["%s|%s" % (a.replace(" ", ","), b.replace(" ", ",")) for a, b, _ in PAIRS])
def test_plans_compare(plans, index):
    a, b, equal = PAIRS[index]
    assert plans[1][2 * index + 1]["same_as_previous"] == str(equal), (a, b)
