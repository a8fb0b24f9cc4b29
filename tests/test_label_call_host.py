"""The host side of the label calls (csrc/dpi_kernels.hip) against what it answered before it was
rewritten around one call record and one workspace tag.  A stand-alone program (tests/label_call_host.hip)
is linked with the library's host units compiled --offload-host-only and defines the HIP runtime calls
they make itself (device memory is host memory, a launch does nothing), so Cha, OU and GBM problems
exist without a GPU and nothing reaches one where there is one.  It prints one line per call;
tests/golden/label_call_host.txt holds the same lines as the previous host code answered them
(profiles/label_call_record/README.md says how they were recorded).  No GPU.

The sweep: every label entry point (dpi_label_prepare, dpi_label_moments, dpi_label_moments_finalize,
dpi_generate_with_gradients, dpi_sample_with_gradients, dpi_label_moments_hessians,
dpi_generate_with_gradients_and_hessians) on a Cha, an OU and a GBM problem with the zero net, with one bad
argument at a time (null handles, n < 0, M = 0, K = 0, epoch = 2^24, m_begin off a block, m_end inside a
block and past M, flags 0 and 8, each null buffer, a workspace one byte short of the size function that
goes with the call, DPI_PREPARED on a pair that stages nothing, a fused-reduce call on a workspace with
no baseline) and the n = 0 forms; the four workspace sizes of those pairs and of the Cha / GBM pairs with
an MLP (the park, the noise staging region); then the workspace tags in the order
tests/test_gpu_label_contract.py takes them on the GPU."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CSRC = ROOT / "deeppicarditeration_amd" / "csrc"
GOLDEN = ROOT / "tests" / "golden" / "label_call_host.txt"
# the host units, and the path units whose launches the sweep reaches (zero nets, GBM MLP [16])
UNITS = ["dpi_kernels.hip", "dpi_net.hip", "dpi_paths_cha.hip", "dpi_paths_ou.hip", "dpi_paths_gbm.hip",
         "dpi_paths_fb_cha.hip", "dpi_paths_fb_ou.hip"]
ENTRIES = ["label_prepare", "label_moments", "label_moments_finalize", "generate_with_gradients",
           "sample_with_gradients", "label_moments_hessians", "generate_with_gradients_and_hessians"]


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    if not Path(HIPCC).exists():
        pytest.fail(f"hipcc not found ({HIPCC})")
    exe = tmp_path_factory.mktemp("label_call_host") / "label_call_host"
    # the other units' launches are never called: their symbols stay unresolved
    subprocess.run([HIPCC, "--offload-host-only", "-O1", "-std=c++17", "-o", str(exe),
                    str(ROOT / "tests" / "label_call_host.hip"), *(str(CSRC / u) for u in UNITS),
                    "-Wl,--unresolved-symbols=ignore-all"], check=True)
    return subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()


def test_label_calls_answer_as_recorded(lines):
    want = GOLDEN.read_text().splitlines()
    assert len(lines) == len(want) <= 1000
    diff = [(g, w) for g, w in zip(lines, want) if g != w]
    assert not diff, f"{len(diff)} lines differ, the first:\n{diff[0][0]}\n{diff[0][1]}"


def test_sweep_reaches_every_entry_point_and_refusal(lines):
    """The golden is not vacuous: every entry point on every kind of problem, both DPI_PREPARED
    refusals, the missing-baseline refusal and each workspace size function's text."""
    rows = [ln.split(" | ") for ln in lines]
    assert {(r[0], r[1]) for r in rows if r[1] in ENTRIES} == {(k, e) for k in ("cha", "ou", "gbm") for e in ENTRIES}
    text = "\n".join(lines)
    for msg in ("without a dpi_label_prepare", "arguments differ", "no dpi_point_baseline", "null problem or net",
                "workspace too small (prepared calls: dpi_workspace_bytes_prepared)",
                "workspace too small (dpi_workspace_bytes_hessians)",
                "workspace too small (dpi_workspace_bytes_hessians_prepared)", "multiple of 64"):
        assert msg in text, msg
    assert sum(r[1] == "sizes" for r in rows) == 5 * 4
