"""What does this checkpoint score on the NYU val / test split?  ``harness.evaluate`` from the command line: every sample of the split goes
through ``DepthEstimationNet.predict`` and ONE launch per batch takes the predicted map and the loader's raw depth to the per-sample metric
sums (``rdm_eval_target_metrics_f64``: resize to 128x128, mask, geometric-mean normalisation and the sums of metrics.py:48-128).  The figures
are the means over the samples of the per-sample values - what the reference's batch-1 validation with Lightning's epoch mean reports
(module.py:99-117) - whatever --batch_size is.

  python -m md_rdm_amd.evaluate --checkpoint last.ckpt --nyu_path /data/nyudepthv2 --split val --out results.json
  python -m md_rdm_amd.evaluate --synthetic 16 --batch_size 8 --precision 16 --out results.json
  python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m md_rdm_amd.evaluate --checkpoint last.ckpt --nyu_path DIR --out results.json

``--split val`` reads the samples through validation_preprocess (Resize + CenterCrop), ``--split test`` through test_preprocess
(dataloaders/nyu.py).  ``--synthetic N`` scores N hash-generated samples instead (``synthetic_samples``).  Under WORLD_SIZE > 1 rank r scores
samples r, r + world, ... (no sample is dropped; the shards may differ in size) and the ranks all-reduce the per-metric sums and the sample
count once at the end; rank 0 prints and writes the result.  ``--rows DIR`` also writes ``row_IIIII.png`` (I = the sample's index) for the first
``--rows_max`` samples of each rank: input | normalised target | the map the metrics saw, the two maps over one colour range (md_rdm_amd.viz).

``--protocol standard`` scores the way the published tables do instead (``metrics.StandardMetrics``, include/rdm_eval.h): linear depth exp(map)
resized to the resolution of the depth the loader returns, valid pixels only (finite, inside (--min_depth, --max_depth) and --crop), a per-image scale
alignment (--align), the aligned prediction clamped to the depth range, and the Eigen et al. error set per image, averaged over the images.
Its figures are NOT comparable with the reference protocol's: ``rmse`` there is the true root mean square, and the deltas are taken of aligned
linear depth.  Images without a valid pixel are left out and counted as ``skipped``.  The rows then show input | raw depth | aligned prediction.
Without --native the command scores at the LOADER's output size (--size, 226x226 by default: the depth after the split's Resize + CenterCrop), and
--crop is in that frame's coordinates.

``--native`` (with --protocol standard and --nyu_path) scores against the RAW depth of every sample instead, at its own resolution: the loader hands
over the depth untouched (``PrefetchLoader(native_depth=True)``) together with the rectangle of that frame which the network input covers (the
split's ``view``; for --split test, Resize(500) -> CenterCrop((480, 640)) leaves rows 9.6 to 470.4 and columns 12.49 to 627.51 of a 480x640 frame), and
the kernel resamples the map over that rectangle (``rdm_eval_standard_view_f64``, include/rdm_eval_view.h).  ``--crop eigen`` is the NYU crop of the
published tables, rows [45, 471) and columns [41, 601) of the 480x640 frame (``--crop garg``: the KITTI crop, fractions of the frame); four integers
still work.  ``--flip`` averages every map with the mirrored map of the mirrored input, the test-time augmentation of those tables, under either
protocol (two passes per batch).  ``--split test --protocol standard --native --crop eigen [--flip]`` therefore gives the 480x640 Eigen-crop figures of
the published NYU tables, with one caveat: a few pixels of the Eigen crop lie outside the view - row 470 of the test transform, whose centre
470.5 is past the view's last row edge 470.4 - and there the prediction is the map's replicated edge, not something the network saw.

``--scale sid`` (standard protocol) adds the metric scale of the d_1 DORN head to every log map before it is scored: the mean log depth of the head's
labels under the ``--sid`` parameter set, ``--sid_offset`` into each bin (``depth.sid_log_scale``).  With ``--align none`` the figures are then those
of METRIC predictions, in the depth's unit.

  python -m md_rdm_amd.evaluate --checkpoint last.ckpt --nyu_path /data/nyudepthv2 --split test --protocol standard --native --crop eigen --flip --out results.json
  python -m md_rdm_amd.evaluate --checkpoint last.ckpt --nyu_path /data/nyudepthv2 --split test --protocol standard --native --align none --scale sid --out results.json
  python -m md_rdm_amd.evaluate --checkpoint last.ckpt --nyu_path /data/nyudepthv2 --split test --protocol standard --crop 8 8 218 218 --out results.json
"""
import json
import os
import sys
from argparse import SUPPRESS, ArgumentParser

# multi-process GPU work on this ROCm stack needs dmabuf IPC (see md_rdm_amd/train.py); must be set before the first HIP call
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

NO_GPU = "md_rdm_amd.evaluate: no GPU is visible to this process (torch.cuda.is_available() is False); evaluation runs on the MI355X only"
CROP_NAMES = ("eigen", "garg")                                                             # metrics.NAMED_CROPS
DEFAULT_METRICS = ["delta1", "delta2", "delta3", "mse", "mae", "log10", "rmse"]            # train.py's --metrics default


class CropNameParser(ArgumentParser):
    """--crop takes four integers; ``--crop eigen`` / ``--crop garg`` is read as the option --crop_name, whose value then stands in ``crop``"""

    def parse_known_args(self, args=None, namespace=None):
        args = list(sys.argv[1:] if args is None else args)
        for i, a in enumerate(args):
            if a == "--crop" and i + 1 < len(args) and args[i + 1] in CROP_NAMES:
                args[i] = "--crop_name"
            elif a.startswith("--crop=") and a[7:] in CROP_NAMES:
                args[i] = "--crop_name=" + a[7:]
        ns, rest = super().parse_known_args(args, namespace)
        if ns.crop_name is not None:
            if ns.crop is not None:
                self.error("argument --crop: given twice, as a name and as four integers")
            ns.crop = ns.crop_name
        del ns.crop_name
        return ns, rest


def build_parser():
    p = CropNameParser("md_rdm_amd.evaluate", description="Score a checkpoint on the NYU val / test split, on the MI355X-native stack")
    p.add_argument("--checkpoint", type=str, default=None, help="Lightning .ckpt or state_dict; without it the hash-filled model is used (a warning says so)")
    p.add_argument("--ema", action="store_true", help="load the checkpoint's averaged weights (state_dict_ema, written by md_rdm_amd.train --ema_decay) instead of the live ones")
    p.add_argument("--nyu_path", type=str, default=None, help="directory of raw NYU samples (.h5 / .npz), as for md_rdm_amd.train")
    p.add_argument("--split", type=str, default="val", choices=["val", "test"])
    p.add_argument("--synthetic", type=int, default=0, metavar="N", help="N hash-generated samples instead of --nyu_path")
    p.add_argument("--batch_size", type=int, default=8)
    p.add_argument("--precision", type=int, default=32, choices=[16, 32], help="32: float32 native plan; 16: bf16 MFMA inference path")
    p.add_argument("--size", type=int, nargs=2, default=[226, 226], metavar=("H", "W"), help="network input size (module.py:19 feeds 226x226)")
    p.add_argument("--relative_decoders", type=int, nargs="*", default=[], help="subset of 6 7 8 9 10, as in md_rdm_amd.train")
    p.add_argument("--metrics", default=list(DEFAULT_METRICS), nargs="+")
    p.add_argument("--exp_pred", action="store_true", help="compare exp(map) with the target instead of the log-domain map: this DEPARTS from the reference, "
                   "which compares the recombination as it is (module.py:117)")
    p.add_argument("--protocol", type=str, default="reference", choices=["reference", "standard"], help="reference: the reference's validation (log-domain map "
                   "against the normalised 128x128 target); standard: aligned full-resolution linear depth, the Eigen et al. error set")
    p.add_argument("--align", type=str, default="median", choices=["none", "median", "logmean"], help="standard protocol: per-image scale alignment")
    p.add_argument("--min_depth", type=float, default=1e-3, help="standard protocol: valid pixels have min_depth < d < max_depth; the prediction is clamped to the range")
    p.add_argument("--max_depth", type=float, default=10.0)
    p.add_argument("--crop", type=int, nargs=4, default=None, metavar=("Y0", "X0", "Y1", "X1"), help="standard protocol: score rows [Y0, Y1) and columns [X0, X1) only; "
                   "or one name in place of the four integers: eigen (NYU: 45 41 471 601 of the 480x640 frame) or garg (KITTI: fractions of the frame)")
    p.add_argument("--crop_name", type=str, default=None, choices=list(CROP_NAMES), help=SUPPRESS)
    p.add_argument("--native", action="store_true", help="standard protocol, --nyu_path: score against every sample's RAW depth at its own resolution, the map "
                   "placed on the part of that frame which the network input covers")
    p.add_argument("--flip", action="store_true", help="average every map with the mirrored map of the mirrored input (two passes per batch)")
    p.add_argument("--scale", type=str, default=None, choices=["sid"], help="standard protocol: add the DORN head's metric log scale to every map (with --align none: metric scores)")
    p.add_argument("--sid", type=str, default=None, metavar="NAME", help="--scale sid: the head's SID parameter set: nyu (default), kitti, floorplan3d, Structured3D")
    p.add_argument("--sid_offset", type=float, default=None, metavar="F", help="--scale sid: position inside a label's bin, 0 (default) = lower edge, 0.5 = centre")
    p.add_argument("--out", type=str, default=None, help="write the result as JSON here")
    p.add_argument("--worker", default=6, type=int, help="threads that decode raw samples (--nyu_path)")
    p.add_argument("--rows", type=str, default=None, metavar="DIR", help="write input | normalised target | prediction PNG rows here")
    p.add_argument("--rows_max", type=int, default=16, metavar="N", help="rows written per rank: the first N samples it scores")
    return p


def synthetic_samples(n, h, w):
    """(x (n,3,h,w) f32, depth (n,1,h,w) f32) for --synthetic: n copies of the margin-searched evaluation input (filler.MARGIN_SEEDS: every
    DORN decision on it holds under the float32 noise of a different batch size or run, at 226x226), each with its own hash-generated depth -
    so the scores do not depend on how the samples are batched."""
    import numpy as np
    from . import filler
    x = filler.synthetic_batch(1, h, w, seed=filler.MARGIN_SEEDS["eval226"])[0]
    y = filler.synthetic_batch(n, h, w)[1]
    return np.ascontiguousarray(np.broadcast_to(x, (n,) + x.shape[1:])), y


def make_computer(args):
    """the metric computer the flags ask for; every refusal is a SystemExit before anything touches a GPU"""
    from .metrics import MetricComputation, StandardMetrics
    try:
        if args.native and args.protocol != "standard":
            raise SystemExit("md_rdm_amd.evaluate: --native needs --protocol standard; the reference protocol scores the normalised 128x128 target")
        if args.native and not args.nyu_path:
            raise SystemExit("md_rdm_amd.evaluate: --native needs --nyu_path: it scores the raw depth of the samples, which --synthetic does not have")
        if args.native and args.rows:
            raise SystemExit("md_rdm_amd.evaluate: --rows with --native is not built: the input shows the view, the raw depth the whole frame")
        if args.scale is not None and args.protocol != "standard":
            raise SystemExit("md_rdm_amd.evaluate: --scale %s needs --protocol standard; the reference protocol compares maps normalised by their geometric mean" % args.scale)
        if (args.sid is not None or args.sid_offset is not None) and args.scale is None:
            raise SystemExit("md_rdm_amd.evaluate: --sid and --sid_offset need --scale sid")
        if args.sid is not None:
            from .depth import SID
            if args.sid not in SID:
                raise SystemExit("md_rdm_amd.evaluate: --sid %s is not one of %s" % (args.sid, ", ".join(SID)))
        if isinstance(args.crop, str) and args.protocol != "standard":
            raise SystemExit("md_rdm_amd.evaluate: --crop %s belongs to --protocol standard; the reference protocol scores the whole 128x128 target" % args.crop)
        if args.protocol == "reference":
            return MetricComputation(args.metrics)
        if args.exp_pred:
            raise SystemExit("md_rdm_amd.evaluate: --exp_pred belongs to --protocol reference; the standard protocol always compares linear depth")
        names = None if list(args.metrics) == DEFAULT_METRICS else args.metrics          # --metrics left alone: the standard list
        H, W = args.size
        if isinstance(args.crop, str):
            if not args.native:                                                           # the depth has the loader's size: the name resolves now
                StandardMetrics(crop=args.crop).resolve_crop(H, W)
        elif args.crop is not None and args.native:                                       # the raw size is not known yet: the kernel checks the frame
            if not (0 <= args.crop[0] < args.crop[2] and 0 <= args.crop[1] < args.crop[3]):
                raise SystemExit("md_rdm_amd.evaluate: --crop %s is empty" % " ".join(map(str, args.crop)))
        elif args.crop is not None and not (0 <= args.crop[0] < args.crop[2] <= H and 0 <= args.crop[1] < args.crop[3] <= W):
            raise SystemExit("md_rdm_amd.evaluate: --crop %s is empty or outside the %dx%d frame" % (" ".join(map(str, args.crop)), H, W))
        return StandardMetrics(names, align=args.align, min_depth=args.min_depth, max_depth=args.max_depth, crop=args.crop)
    except KeyError as e:
        raise SystemExit("md_rdm_amd.evaluate: %s" % e.args[0])
    except ValueError as e:
        raise SystemExit("md_rdm_amd.evaluate: %s" % e)


def shard(indices, rank, world):
    """rank r of `world` takes indices[r::world]: every sample exactly once, shards of unequal size allowed"""
    return list(indices)[rank::world]


def main(argv=None):
    args = build_parser().parse_args(argv)
    if bool(args.synthetic) == bool(args.nyu_path):
        raise SystemExit("md_rdm_amd.evaluate: give --nyu_path DIR or --synthetic N (not both)")
    if args.batch_size < 1:
        raise SystemExit("md_rdm_amd.evaluate: --batch_size must be positive")
    if args.ema and not args.checkpoint:
        raise SystemExit("md_rdm_amd.evaluate: --ema needs --checkpoint: the averaged weights are an entry of a checkpoint")
    if args.synthetic < 0:
        raise SystemExit("md_rdm_amd.evaluate: --synthetic must be positive")
    if args.rows_max < 0:
        raise SystemExit("md_rdm_amd.evaluate: --rows_max must not be negative")
    computer = make_computer(args)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit(NO_GPU)
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    import torch.distributed as dist
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=dev)

    from . import checkpoint, filler, harness
    from .network.RDM_Net import DepthEstimationNet
    model = DepthEstimationNet(relative_decoders=tuple(args.relative_decoders))
    if args.checkpoint:
        try:
            checkpoint.from_lightning(model, args.checkpoint, ema=args.ema)
        except checkpoint.NoAveragedWeights as e:                 # --ema on a checkpoint without averaged weights
            raise SystemExit("md_rdm_amd.evaluate: %s" % e.args[0])
    else:
        if rank == 0:
            print("warning: no --checkpoint: using the deterministic hash-filled weights (filler.fill_state_dict) - the scores mean nothing", flush=True)
        filler.fill_state_dict(model.state_dict())
    model = model.to(dev).eval().set_precision("bf16" if args.precision == 16 else "f32")
    H, W = args.size
    native = {"view": None, "crop": None}                                # --native: of the last batch this rank scored

    if args.synthetic:
        xs, ys = synthetic_samples(args.synthetic, H, W)
        mine = shard(range(args.synthetic), rank, world)

        def batches():
            for i in range(0, len(mine), args.batch_size):
                idx = mine[i:i + args.batch_size]
                yield torch.from_numpy(xs[idx]).to(dev), torch.from_numpy(ys[idx]).to(dev)
        source = "synthetic"
    else:
        from .dataloaders import NYUDataset, PrefetchLoader
        ds = NYUDataset(args.nyu_path, split=args.split, output_size=(H, W))
        loader = PrefetchLoader(ds, args.batch_size, shuffle=False, device=dev, drop_last=False, rank=rank, world=world, workers=args.worker,
                                indices=range(len(ds)), native_depth=args.native)

        def batches():
            for x, y in loader:
                if args.native:
                    computer.view = loader.view                          # this batch's raw frame
                    native.update(view=list(loader.view), crop=computer.resolve_crop(y.shape[2], y.shape[3]))
                yield x, y
        source = args.split
    rows = []
    result = harness.evaluate(model, batches(), computer, exp_pred=args.exp_pred, rows_out=rows if args.rows else None, rows_max=args.rows_max, flip=args.flip,
                              **(dict(scale=args.scale, sid=args.sid or "nyu", sid_offset=args.sid_offset or 0.0) if args.scale else {}))
    if args.rows:
        from . import viz
        os.makedirs(args.rows, exist_ok=True)
        for i, row in enumerate(rows):                                   # rank r scored samples r, r + world, ... in order
            viz.write_png(os.path.join(args.rows, "row_%05d.png" % (rank + i * world)), row)
    if world > 1:
        dist.destroy_process_group()
    if rank == 0:
        for name in computer.names:
            print("%s %.6f" % (name, result[name]), flush=True)
        print("n %d" % result["n"], flush=True)
        standard = args.protocol == "standard"
        if standard:
            print("skipped %d" % result["skipped"], flush=True)
        if args.out:
            record = {"split": source, "n": result["n"], "batch_size": args.batch_size, "precision": args.precision, "size": [H, W], "exp_pred": bool(args.exp_pred),
                      "relative_decoders": list(args.relative_decoders), "checkpoint": args.checkpoint, "world": world,
                      "metrics": {name: result[name] for name in computer.names}, "protocol": args.protocol}
            if standard:
                crop = native["crop"] if args.native else computer.resolve_crop(H, W)          # a named crop as its integers
                record.update(align=args.align, min_depth=args.min_depth, max_depth=args.max_depth, crop=list(crop) if crop else None,
                              skipped=result["skipped"], native=bool(args.native), view=native["view"], flip=bool(args.flip))
                if args.scale:
                    record.update(scale=args.scale, sid=args.sid or "nyu", sid_offset=args.sid_offset or 0.0)
            elif args.flip:
                record["flip"] = True
            d = os.path.dirname(os.path.abspath(args.out))
            os.makedirs(d, exist_ok=True)
            with open(args.out, "w") as fh:
                json.dump(record, fh, indent=1)
                fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
