"""`python -m md_rdm_amd.predict` without a GPU: the flags parse, and a machine with no visible device gets one clear line, not a traceback."""
import os
import subprocess
import sys

from conftest import ROOT


def test_help_names_the_flags():
    from md_rdm_amd import predict
    text = predict.build_parser().format_help()
    for flag in ("--checkpoint", "--precision", "--batch_size", "--size", "--out", "--linear", "--full_res", "--synthetic"):
        assert flag in text, flag
    args = predict.build_parser().parse_args(["--out", "d", "--synthetic", "3", "--precision", "16", "--size", "228", "304", "--linear", "--full_res"])
    assert (args.synthetic, args.precision, args.size, args.linear, args.full_res, args.batch_size, args.checkpoint) == (3, 16, [228, 304], True, True, 8, None)
    assert predict.build_parser().parse_args(["--out", "d", "a.npy", "b.npz"]).inputs == ["a.npy", "b.npz"]
    r = subprocess.run([sys.executable, "-m", "md_rdm_amd.predict", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")))
    assert r.returncode == 0 and "--full_res" in r.stdout


def test_no_visible_gpu_is_one_clear_line(tmp_path):
    from md_rdm_amd import predict
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "md_rdm_amd.predict", "--synthetic", "1", "--out", str(tmp_path / "maps")], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "Traceback" not in r.stderr
    lines = [l for l in r.stderr.splitlines() if l.strip()]
    assert lines and lines[-1] == predict.NO_GPU and "no GPU is visible" in predict.NO_GPU
    assert not (tmp_path / "maps").exists() or not os.listdir(tmp_path / "maps")
