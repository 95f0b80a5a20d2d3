"""Image in, depth map out: ``DepthEstimationNet.predict`` from the command line.  The reference has no such command; what it computes for
an image without a target is ``recombination(model(x)[0])`` (network/computations.py:394-421, :499-510), a 128x128 map of log relative depth.

  python -m md_rdm_amd.predict --checkpoint last.ckpt --out maps frame0.npy frame1.png
  python -m md_rdm_amd.predict --synthetic 8 --precision 16 --batch_size 8 --out maps

Inputs are uint8 HxWx3 frames: ``.npy`` files, ``.npz`` files (array ``rgb``, else the first array) and, where Pillow is installed,
ordinary image files.  They pass through the GPU test transform of dataloaders/nyu.py (Resize(500) -> CenterCrop((480, 640)) ->
Resize(--size)); at least 480x640 after the first resize, like the reference's test_preprocess.  ``--synthetic N`` feeds N hash-generated
network inputs (filler.synthetic_batch) of --size instead.  One ``.npy`` per input lands in --out: the (1,128,128) float64 log map,
float32 ``exp`` of it with --linear, resized to the frame region the network saw ((480, 640), or --size for synthetic inputs) with --full_res.
``--png`` writes ``NAME.png`` beside each ``.npy``: the saved map in jet colours (md_rdm_amd.viz, one launch per batch), over its own range or
over ``--png_range LO HI`` (comparable frames); ``--png_with_input`` puts the network input to its left, the map resized to the input's size.
``--flip`` averages every log map with the mirrored map of the mirrored input (``predict(x, flip=True)``: two passes per batch).

``--metric`` writes depth in metres instead (md_rdm_amd.depth, one launch per batch): the scale is the mean log depth of the d_1 DORN head's
labels under the ``--sid`` parameter set (``--sid_offset 0.5``: bin centres instead of lower bin edges), and the ``.npy`` is the float32
(1,h,w) frame - 128x128, the --full_res region, or with ``--native`` the input frame's own shape, the map placed on the rectangle of it the
network saw (``nyu.test_view``; the pixels outside are 0, "no measurement", or with ``--outside edge`` the map's replicated edge).
``--png16`` also writes ``NAME_depth.png``, the 16-bit greyscale depth PNG downstream tools read, in steps of ``--depth_unit`` metres
(default 0.001: millimetres; 65535 saturates).  ``--png`` then colours the saved metric map.

  python -m md_rdm_amd.predict --checkpoint last.ckpt --out maps --metric --native --png16 frame0.npy

``--ply`` (with --metric) also writes ``NAME.ply``: the saved metric frame as a binary little-endian point cloud (md_rdm_amd.cloud, one launch
per batch), pixels without a measurement or outside ``--min_depth`` / ``--max_depth`` dropped, every ``--ply_step``-th pixel of every
``--ply_step``-th row, with unit normals facing the camera under ``--ply_normals``.  The camera is ``--camera nyu`` (the default) or
``--intrinsics FX FY CX CY``, always the intrinsics of the RAW frame: with ``--native`` they are used as they are and the points carry the input
frame's colours; otherwise they are mapped to the saved frame through the rectangle of the raw frame it shows (``cloud.intrinsics_in_view`` of
``nyu.test_view``) and the cloud has no colour.  For ``--synthetic`` inputs the raw frame is the network input itself.

  python -m md_rdm_amd.predict --checkpoint last.ckpt --out maps --metric --native --ply --ply_normals frame0.npy

``--refine`` (with --metric --native) filters the metric frame under the raw input frame before anything is written (md_rdm_amd.refine, a joint
bilateral filter, one launch per batch): taps whose colour differs from the pixel's get little weight, so the depth edges that the enlargement of the
128x128 map has smeared move back to the colour edges.  ``--refine_radius R`` / ``--refine_step S`` give (2R + 1)^2 taps at multiples of S pixels
(R <= 8, S <= 16, R * S <= 24; default 3 and 4), ``--refine_sigma_space`` (default R * S / 2) and ``--refine_sigma_color`` (default 12) the two
widths; ``--refine_fill`` also fills pixels without a measurement from their valid taps.  The ``.npy``, ``NAME_depth.png`` and ``NAME.ply`` all come
from the refined planes.  The defaults are a starting point: their effect on depth accuracy has not been measured.

  python -m md_rdm_amd.predict --checkpoint last.ckpt --out maps --metric --native --refine --png16 --ply frame0.npy

``--mesh`` (with --metric --ply) gives ``NAME.ply`` a face element as well (md_rdm_amd.mesh, two more launches per batch): the pixel grid of the
saved frame triangulated, two triangles per cell, without the triangles that touch a dropped pixel or whose largest depth exceeds
``--mesh_edge_ratio R`` times their smallest (R >= 1, default 1.05; ``inf`` keeps every triangle of valid pixels) - the sheets a surface would
otherwise draw across every depth step.  The vertices are the cloud's points, unchanged; ``--ply_step N`` decimates the mesh with them.  The
default ratio is a starting point: its effect has not been measured on real predictions.

  python -m md_rdm_amd.predict --checkpoint last.ckpt --out maps --metric --native --refine --ply --ply_normals --mesh --mesh_edge_ratio 1.1 frame0.npy

``--stereo M`` (with --metric) also writes ``NAME_right.png``: the saved frame and its colours seen from a camera M metres to the right
(md_rdm_amd.warp, three more launches per batch: a z-buffered forward warp, the nearest surface kept in every pixel) - with the input the right eye
of a stereo pair; with ``--png16`` also ``NAME_right_depth.png``, the warped depth in steps of ``--depth_unit``.  ``--view_pose`` takes the twelve
values r00 r01 r02 t0 r10 .. t2 of a pose [R | t] from the saved frame's camera to any other and writes ``NAME_view.png`` (and
``NAME_view_depth.png``) likewise.  The picture has the saved frame's shape and intrinsics (``--camera`` / ``--intrinsics``, ``--min_depth`` /
``--max_depth`` as for --ply) and needs the saved frame's colours: ``--native`` for file inputs; for ``--synthetic`` inputs ``--full_res``, which
saves the frame at the network input's own size, whose values are then the colours.  ``--view_splat S`` lets every point cover S x S pixels
(1..4, default 1) and ``--view_fill F`` fills holes of up to about 2F pixels along each row from the farther side (0..64, default 8); pixels no
point reached stay black.  With ``--refine`` the refined planes are warped.  Both defaults are starting points: their effect has not been measured
on real predictions.

  python -m md_rdm_amd.predict --checkpoint last.ckpt --out maps --metric --native --stereo 0.06 --png16 frame0.npy
  python -m md_rdm_amd.predict --synthetic 2 --out maps --metric --full_res --stereo 0.06

``--anchors PATH...`` (with --metric --native; for ``--synthetic`` inputs with --full_res) ties every frame to metric measurements of it
(md_rdm_amd.anchor, three launches per batch): one file per input, in the saved frame's own geometry, a pixel without a measurement 0 - SLAM / SfM
landmarks rendered into the frame, a LiDAR sweep, a sensor frame with holes.  ``.npy`` files hold float32 metres; 16-bit greyscale PNGs hold steps
of ``--anchor_unit`` metres (default 0.001) and are read with the standard library.  The SID scale becomes the prior;
``--anchor_fit logmean`` (the default) adds the mean log residual of the anchors to it, ``median`` replaces it by the ratio of medians
(``evaluate --align median``'s statistic), ``none`` keeps it.  What the scale leaves is summed over cells of ``--anchor_cell`` pixels (default 16),
smoothed over ``--anchor_sigma`` cells (default 2) and added as a correction field, pulled to 0 by ``--anchor_lambda`` (default 1, in anchors) where
there are few anchors; ``--anchor_no_field`` fits the scale alone.  ``--anchor_reject F`` drops anchors whose log residual against the prior exceeds
F (``median`` makes a prior that outliers do not move).  ``--min_depth`` / ``--max_depth`` bound the anchors too.  The ``.npy``, ``NAME_depth.png``,
``NAME.ply`` and ``NAME_right.png`` all come from the anchored planes; with ``--refine`` the anchored plane is filtered.  The defaults are starting
points: their effect on real data has not been measured.

  python -m md_rdm_amd.predict --checkpoint last.ckpt --out maps --metric --native --anchors frame0_lidar.png --anchor_fit median --anchor_reject 0.5 frame0.npy

``--fuse --poses FILE`` (with --metric --native; for ``--synthetic`` inputs with --full_res) also writes ONE ``fused.ply`` for the whole sequence
(md_rdm_amd.fuse): every batch's saved frames and their colours are integrated into one truncated signed distance volume (one launch per batch),
and after the last batch the volume's surface is read out as oriented, coloured points in world coordinates (three more launches, twice).  ``FILE``
is a ``.npy`` or a text file with one row of twelve values r00 r01 r02 t0 r10 .. t2 per input frame, in input order: the pose [R | t] from WORLD to
that frame's camera, or with ``--poses_c2w`` from the camera to the world (what SLAM systems write; inverted on the host in float64).  The volume
has voxels of ``--fuse_voxel`` metres (default 0.02) and a truncation of ``--fuse_trunc`` metres (default 4 voxels); ``--fuse_origin X Y Z`` and
``--fuse_dims NX NY NZ`` place it, and what is not given comes from the box of the cameras' frusta up to ``--max_depth`` (``fuse.bounds``), which
must then be given.  A voxel counts once its weight reaches ``--fuse_min_weight`` (default 1: one frame); ``--fuse_max_weight`` caps the running
weight (default 64).  ``--camera`` / ``--intrinsics`` and ``--min_depth`` / ``--max_depth`` are --ply's; ``--ply_normals`` gives the points
normals; with ``--anchors`` the anchored frames and with ``--refine`` the refined ones are fused - unanchored monocular frames disagree in scale and
blur the surface.  The defaults are starting points: their effect on real data has not been measured.

  python -m md_rdm_amd.predict --checkpoint last.ckpt --out maps --metric --native --anchors a0.png a1.png --fuse --poses poses.txt --poses_c2w --max_depth 6 f0.npy f1.npy
"""
import os
import sys
import time
from argparse import ArgumentParser

NO_GPU = "md_rdm_amd.predict: no GPU is visible to this process (torch.cuda.is_available() is False); the predict path runs on the MI355X only"


def build_parser():
    p = ArgumentParser("md_rdm_amd.predict", description="Depth maps (log relative depth, 128x128) for images, on the MI355X-native stack")
    p.add_argument("inputs", nargs="*", help=".npy / .npz uint8 HxWx3 frames, or image files (needs Pillow)")
    p.add_argument("--checkpoint", type=str, default=None, help="Lightning .ckpt or state_dict; without it the hash-filled model is used (a warning says so)")
    p.add_argument("--ema", action="store_true", help="load the checkpoint's averaged weights (state_dict_ema, written by md_rdm_amd.train --ema_decay) instead of the live ones")
    p.add_argument("--precision", type=int, default=32, choices=[16, 32], help="32: float32 native plan; 16: bf16 MFMA inference path")
    p.add_argument("--batch_size", type=int, default=8)
    p.add_argument("--size", type=int, nargs=2, default=[226, 226], metavar=("H", "W"), help="network input size (module.py:19 feeds 226x226)")
    p.add_argument("--out", type=str, required=True, help="directory for the .npy maps")
    p.add_argument("--linear", action="store_true", help="write float32 exp(map) instead of the float64 log map")
    p.add_argument("--full_res", action="store_true", help="bicubic resize of the log map to the frame region the network saw (480x640; --size for --synthetic)")
    p.add_argument("--flip", action="store_true", help="average every map with the mirrored map of the mirrored input (log domain, before --linear and --full_res; "
                   "two passes per batch)")
    p.add_argument("--synthetic", type=int, default=0, metavar="N", help="N hash-generated inputs (filler.synthetic_batch) instead of files")
    p.add_argument("--relative_decoders", type=int, nargs="*", default=[], help="subset of 6 7 8 9 10, as in md_rdm_amd.train")
    p.add_argument("--png", action="store_true", help="also write NAME.png: the saved map in jet colours (honours --linear and --full_res)")
    p.add_argument("--png_range", type=float, nargs=2, default=None, metavar=("LO", "HI"), help="fixed colour range instead of each map's own minimum / maximum")
    p.add_argument("--png_with_input", action="store_true", help="the .png shows input | map, the map resized to the network input's size")
    p.add_argument("--metric", action="store_true", help="write float32 depth in metres, the scale taken from the ordinal (DORN) head")
    p.add_argument("--sid", type=str, default=None, metavar="NAME", help="--metric: the head's SID parameter set: nyu (default), kitti, floorplan3d, Structured3D")
    p.add_argument("--sid_offset", type=float, default=None, metavar="F", help="--metric: position inside a label's bin, 0 (default) = lower edge, 0.5 = centre")
    p.add_argument("--native", action="store_true", help="--metric, file inputs: the output has the input frame's own shape, the map placed on the part the network saw")
    p.add_argument("--outside", type=str, default=None, choices=["zero", "edge"], help="--metric: pixels outside the view are 0 (default) or the map's replicated edge")
    p.add_argument("--png16", action="store_true", help="--metric: also write NAME_depth.png, 16-bit greyscale in steps of --depth_unit")
    p.add_argument("--depth_unit", type=float, default=None, metavar="M", help="--metric: metres per step of the 16-bit PNG (default 0.001)")
    p.add_argument("--ply", action="store_true", help="--metric: also write NAME.ply, the metric frame as a binary point cloud")
    p.add_argument("--ply_normals", action="store_true", help="--ply: unit normals facing the camera, from the neighbouring pixels")
    p.add_argument("--ply_step", type=int, default=None, metavar="N", help="--ply: every N-th pixel of every N-th row (default 1)")
    p.add_argument("--camera", type=str, default=None, metavar="NAME", help="--ply: a named intrinsics set of the raw frame: nyu (default)")
    p.add_argument("--intrinsics", type=float, nargs=4, default=None, metavar=("FX", "FY", "CX", "CY"), help="--ply: pinhole intrinsics of the raw frame, instead of --camera")
    p.add_argument("--min_depth", type=float, default=None, metavar="M", help="--ply: drop points nearer than M metres (default 0)")
    p.add_argument("--max_depth", type=float, default=None, metavar="M", help="--ply: drop points farther than M metres (default: no limit)")
    p.add_argument("--refine", action="store_true", help="--metric --native: filter the metric frame under the input frame (joint bilateral) before it is written")
    p.add_argument("--refine_radius", type=int, default=None, metavar="R", help="--refine: (2R + 1)^2 taps, 1 <= R <= 8 (default 3)")
    p.add_argument("--refine_step", type=int, default=None, metavar="S", help="--refine: the taps are S pixels apart, 1 <= S <= 16 and R * S <= 24 (default 4)")
    p.add_argument("--refine_sigma_space", type=float, default=None, metavar="F", help="--refine: width of the spatial weight in pixels (default R * S / 2)")
    p.add_argument("--refine_sigma_color", type=float, default=None, metavar="F", help="--refine: width of the colour weight in steps of the 8-bit guide (default 12)")
    p.add_argument("--refine_fill", action="store_true", help="--refine: pixels without a measurement take the weighted mean of their valid taps; with the default "
                   "--outside zero the band of such pixels within R * S of the view is filled from inside it")
    p.add_argument("--mesh", action="store_true", help="--ply: NAME.ply also carries triangles: the pixel grid without the faces across depth steps")
    p.add_argument("--mesh_edge_ratio", type=float, default=None, metavar="R", help="--mesh: drop a triangle whose largest depth exceeds R times its smallest, R >= 1 "
                   "(default 1.05, a starting point; inf keeps all)")
    p.add_argument("--stereo", type=float, default=None, metavar="M", help="--metric, with --native or --synthetic --full_res: also write NAME_right.png, the frame seen "
                   "from a camera M metres to the right")
    p.add_argument("--view_pose", type=float, nargs=12, default=None, metavar="P", help="--metric, with --native or --synthetic --full_res: also write NAME_view.png, the frame "
                   "seen under the pose r00 r01 r02 t0 r10 r11 r12 t1 r20 r21 r22 t2 (saved frame's camera -> the other camera, metres)")
    p.add_argument("--view_splat", type=int, default=None, metavar="S", help="--stereo / --view_pose: every point covers S x S pixels, 1..4 (default 1, a starting point)")
    p.add_argument("--view_fill", type=int, default=None, metavar="F", help="--stereo / --view_pose: fill holes from the farther of the nearest pixels within F columns, 0..64 "
                   "(default 8, a starting point)")
    p.add_argument("--anchors", type=str, nargs="+", default=None, metavar="PATH", help="--metric --native (or --synthetic --full_res): one frame of metric measurements "
                   "per input, .npy float32 metres or a 16-bit PNG in steps of --anchor_unit, 0 = no measurement; the frames are fitted to them")
    p.add_argument("--anchor_fit", type=str, default=None, choices=["logmean", "median", "none"], help="--anchors: how the scale is fitted (default logmean)")
    p.add_argument("--anchor_cell", type=int, default=None, metavar="N", help="--anchors: side of the correction field's cells in pixels (default 16, a starting point)")
    p.add_argument("--anchor_sigma", type=float, default=None, metavar="F", help="--anchors: width of the field's smoothing in cells (default 2, a starting point)")
    p.add_argument("--anchor_lambda", type=float, default=None, metavar="F", help="--anchors: regulariser of the field in anchors (default 1, a starting point)")
    p.add_argument("--anchor_reject", type=float, default=None, metavar="F", help="--anchors: drop anchors whose log residual against the prior exceeds F (default: none)")
    p.add_argument("--anchor_unit", type=float, default=None, metavar="M", help="--anchors: metres per step of a 16-bit PNG anchor file (default 0.001)")
    p.add_argument("--anchor_no_field", action="store_true", help="--anchors: fit the scale only, no correction field")
    p.add_argument("--fuse", action="store_true", help="--metric, with --native or --synthetic --full_res: integrate every saved frame into one TSDF volume and write "
                   "fused.ply, its surface as oriented points in world coordinates; needs --poses")
    p.add_argument("--poses", type=str, default=None, metavar="FILE", help="--fuse: .npy or text, one row of twelve values r00 r01 r02 t0 .. t2 per input frame: world -> camera")
    p.add_argument("--poses_c2w", action="store_true", help="--fuse: the rows of --poses are camera -> world and are inverted")
    p.add_argument("--fuse_voxel", type=float, default=None, metavar="M", help="--fuse: the voxels' side in metres (default 0.02, a starting point: its effect on real "
                   "data has not been measured)")
    p.add_argument("--fuse_trunc", type=float, default=None, metavar="M", help="--fuse: the truncation distance in metres (default 4 voxels, a starting point, not measured)")
    p.add_argument("--fuse_dims", type=int, nargs=3, default=None, metavar=("NX", "NY", "NZ"), help="--fuse: the volume's voxels (default: the box of the frusta up to --max_depth)")
    p.add_argument("--fuse_origin", type=float, nargs=3, default=None, metavar=("X", "Y", "Z"), help="--fuse: the centre of voxel (0, 0, 0) in world metres (default: the "
                   "box of the frusta up to --max_depth)")
    p.add_argument("--fuse_min_weight", type=float, default=None, metavar="W", help="--fuse: a voxel counts from this weight on (default 1: seen by one frame; a starting "
                   "point, not measured)")
    p.add_argument("--fuse_max_weight", type=float, default=None, metavar="W", help="--fuse: the cap of a voxel's running weight, >= 1 (default 64)")
    return p


def check_png_args(args):
    """the --png* flags' own rules; raises SystemExit"""
    if (args.png_range is not None or args.png_with_input) and not args.png:
        raise SystemExit("md_rdm_amd.predict: --png_range and --png_with_input need --png")
    if args.png_range is not None and not args.png_range[0] < args.png_range[1]:
        raise SystemExit("md_rdm_amd.predict: --png_range needs LO < HI (got %r %r)" % tuple(args.png_range))


def check_metric_args(args):
    """the metric flags' own rules; raises SystemExit"""
    if not args.metric:
        given = [f for f, v in (("--png16", args.png16), ("--sid", args.sid is not None), ("--sid_offset", args.sid_offset is not None),
                                ("--outside", args.outside is not None), ("--depth_unit", args.depth_unit is not None), ("--native", args.native)) if v]
        if given:
            raise SystemExit("md_rdm_amd.predict: --png16, --sid, --sid_offset, --outside, --depth_unit and --native need --metric (got %s)" % " ".join(given))
        return
    if args.native and (args.full_res or args.synthetic):
        raise SystemExit("md_rdm_amd.predict: --native excludes --full_res and --synthetic: it places the map on the raw frame of a file input")
    if args.linear:
        raise SystemExit("md_rdm_amd.predict: --metric excludes --linear: the metric map is linear depth already")
    from .depth import SID
    if args.sid is not None and args.sid not in SID:
        raise SystemExit("md_rdm_amd.predict: --sid %s is not one of %s" % (args.sid, ", ".join(SID)))
    if args.depth_unit is not None and not 0 < args.depth_unit < float("inf"):
        raise SystemExit("md_rdm_amd.predict: --depth_unit must be positive and finite (got %r)" % args.depth_unit)


def check_ply_args(args):
    """the --ply flags' own rules; raises SystemExit"""
    import math
    view = args.stereo is not None or args.view_pose is not None          # the novel views take the camera and the depth range too
    anchored = args.anchors is not None                                   # ... and the anchors the depth range
    if args.fuse:                                                         # ... and the fused volume both, and --ply_normals for its points
        view = anchored = True
    if not args.ply:
        given = [f for f, v in (("--ply_normals", args.ply_normals and not args.fuse), ("--ply_step", args.ply_step is not None), ("--camera", args.camera is not None and not view),
                                ("--intrinsics", args.intrinsics is not None and not view), ("--min_depth", args.min_depth is not None and not view and not anchored),
                                ("--max_depth", args.max_depth is not None and not view and not anchored)) if v]
        if given:
            raise SystemExit("md_rdm_amd.predict: --ply_normals, --ply_step, --camera, --intrinsics, --min_depth and --max_depth need --ply (got %s)" % " ".join(given))
        if not view and not anchored:
            return
    if args.ply and not args.metric:
        raise SystemExit("md_rdm_amd.predict: --ply needs --metric: a point cloud is made of depth in metres")
    if args.camera is not None and args.intrinsics is not None:
        raise SystemExit("md_rdm_amd.predict: give --camera or --intrinsics (not both)")
    from .cloud import INTRINSICS
    if args.camera is not None and args.camera not in INTRINSICS:
        raise SystemExit("md_rdm_amd.predict: --camera %s is not one of %s" % (args.camera, ", ".join(INTRINSICS)))
    if args.intrinsics is not None and not (all(math.isfinite(v) for v in args.intrinsics) and args.intrinsics[0] != 0 and args.intrinsics[1] != 0):
        raise SystemExit("md_rdm_amd.predict: --intrinsics must be finite with FX and FY not 0 (got %r)" % (args.intrinsics,))
    if args.ply_step is not None and args.ply_step < 1:
        raise SystemExit("md_rdm_amd.predict: --ply_step must be positive (got %d)" % args.ply_step)
    lo, hi = args.min_depth if args.min_depth is not None else 0.0, args.max_depth if args.max_depth is not None else math.inf
    if not lo >= 0:
        raise SystemExit("md_rdm_amd.predict: --min_depth must be >= 0 (got %r)" % lo)
    if not hi >= lo:
        raise SystemExit("md_rdm_amd.predict: --max_depth must not be below --min_depth (got %r, %r)" % (hi, lo))


def check_refine_args(args):
    """the --refine flags' own rules (the ranges are the library's, include/rdm_refine.h); raises SystemExit"""
    if not args.refine:
        given = [f for f, v in (("--refine_radius", args.refine_radius is not None), ("--refine_step", args.refine_step is not None),
                                ("--refine_sigma_space", args.refine_sigma_space is not None), ("--refine_sigma_color", args.refine_sigma_color is not None),
                                ("--refine_fill", args.refine_fill)) if v]
        if given:
            raise SystemExit("md_rdm_amd.predict: --refine_radius, --refine_step, --refine_sigma_space, --refine_sigma_color and --refine_fill need --refine (got %s)" % " ".join(given))
        return
    if not (args.metric and args.native):
        raise SystemExit("md_rdm_amd.predict: --refine needs --metric --native: the guide is the raw frame, which only that mode has at the output's geometry")
    from .refine import DEFAULTS, check_params
    bad = check_params(args.refine_radius if args.refine_radius is not None else DEFAULTS["radius"], args.refine_step if args.refine_step is not None else DEFAULTS["step"],
                       args.refine_sigma_space, args.refine_sigma_color if args.refine_sigma_color is not None else DEFAULTS["sigma_color"])
    if bad:
        raise SystemExit("md_rdm_amd.predict: --refine: " + bad)


def check_mesh_args(args):
    """the --mesh flags' own rules (the range is the library's, include/rdm_mesh.h); raises SystemExit"""
    if not args.mesh:
        if args.mesh_edge_ratio is not None:
            raise SystemExit("md_rdm_amd.predict: --mesh_edge_ratio needs --mesh")
        return
    if not args.ply:
        raise SystemExit("md_rdm_amd.predict: --mesh needs --ply: the faces go into NAME.ply, behind the cloud's points")
    if args.mesh_edge_ratio is not None and not args.mesh_edge_ratio >= 1:
        raise SystemExit("md_rdm_amd.predict: --mesh_edge_ratio must be >= 1 and not NaN (got %r)" % args.mesh_edge_ratio)


def check_view_args(args):
    """the --stereo / --view_* flags' own rules (the ranges are the library's, include/rdm_warp.h); raises SystemExit"""
    import math
    if args.stereo is None and args.view_pose is None:
        given = [f for f, v in (("--view_splat", args.view_splat is not None), ("--view_fill", args.view_fill is not None)) if v]
        if given:
            raise SystemExit("md_rdm_amd.predict: --view_splat and --view_fill need --stereo or --view_pose (got %s)" % " ".join(given))
        return
    if not args.metric:
        raise SystemExit("md_rdm_amd.predict: --stereo and --view_pose need --metric: a view is rendered from depth in metres")
    if not (args.native or (args.synthetic and args.full_res)):
        raise SystemExit("md_rdm_amd.predict: --stereo and --view_pose need the colours of the saved frame: --native for file inputs, --full_res for --synthetic "
                         "inputs (the frame is then the network input itself)")
    if args.stereo is not None and not math.isfinite(args.stereo):
        raise SystemExit("md_rdm_amd.predict: --stereo must be finite (got %r)" % args.stereo)
    if args.view_pose is not None and not all(math.isfinite(v) for v in args.view_pose):
        raise SystemExit("md_rdm_amd.predict: --view_pose must be twelve finite values (got %r)" % (args.view_pose,))
    from .warp import FILL, SPLAT, check_params
    bad = check_params(args.view_splat if args.view_splat is not None else SPLAT, args.view_fill if args.view_fill is not None else FILL)
    if bad:
        raise SystemExit("md_rdm_amd.predict: --view_splat / --view_fill: " + bad)


def check_anchor_args(args):
    """the --anchor* flags' own rules (the ranges are the library's, include/rdm_anchor.h); raises SystemExit"""
    import math
    if args.anchors is None:
        given = [f for f, v in (("--anchor_fit", args.anchor_fit is not None), ("--anchor_cell", args.anchor_cell is not None), ("--anchor_sigma", args.anchor_sigma is not None),
                                ("--anchor_lambda", args.anchor_lambda is not None), ("--anchor_reject", args.anchor_reject is not None),
                                ("--anchor_unit", args.anchor_unit is not None), ("--anchor_no_field", args.anchor_no_field)) if v]
        if given:
            raise SystemExit("md_rdm_amd.predict: --anchor_fit, --anchor_cell, --anchor_sigma, --anchor_lambda, --anchor_reject, --anchor_unit and --anchor_no_field need "
                             "--anchors (got %s)" % " ".join(given))
        return
    if not args.metric:
        raise SystemExit("md_rdm_amd.predict: --anchors needs --metric: the anchors are depth in metres")
    if not (args.native or (args.synthetic and args.full_res)):
        raise SystemExit("md_rdm_amd.predict: --anchors needs the saved frame in the anchors' geometry: --native for file inputs, --full_res for --synthetic "
                         "inputs (the frame is then the network input itself)")
    n_in = args.synthetic or len(args.inputs)
    if len(args.anchors) != n_in:
        raise SystemExit("md_rdm_amd.predict: --anchors takes one file per input (got %d files for %d inputs)" % (len(args.anchors), n_in))
    if args.anchor_unit is not None and not 0 < args.anchor_unit < math.inf:
        raise SystemExit("md_rdm_amd.predict: --anchor_unit must be positive and finite (got %r)" % args.anchor_unit)
    from .anchor import DEFAULTS, check_params
    bad = check_params(args.anchor_cell if args.anchor_cell is not None else DEFAULTS["cell"], args.anchor_sigma if args.anchor_sigma is not None else DEFAULTS["sigma"],
                       args.anchor_lambda if args.anchor_lambda is not None else DEFAULTS["lam"], args.anchor_reject)
    if bad:
        raise SystemExit("md_rdm_amd.predict: --anchors: " + bad)


def load_poses(path):
    """(N,12) float64 rows of a .npy ((N,12), (N,3,4) or (N,4,4)) or of a text file with twelve values per row"""
    import numpy as np
    try:
        p = np.load(path) if os.path.splitext(path)[1].lower() == ".npy" else np.loadtxt(path, dtype=np.float64, ndmin=2)
        p = np.asarray(p, np.float64)
    except (OSError, ValueError) as e:
        raise SystemExit("md_rdm_amd.predict: --poses %s: %s" % (path, e))
    if p.ndim == 3 and p.shape[1:] in ((3, 4), (4, 4)):
        p = p[:, :3, :].reshape(-1, 12)
    if p.ndim != 2 or p.shape[1] != 12 or not np.isfinite(p).all():
        raise SystemExit("md_rdm_amd.predict: --poses %s: need rows of twelve finite values [R | t], got an array of shape %s" % (path, p.shape))
    return np.ascontiguousarray(p)


def check_fuse_args(args):
    """the --fuse flags' own rules (the ranges are the library's, include/rdm_fuse.h); raises SystemExit.  -> the (N,12) world-to-camera poses, or None"""
    import math
    if not args.fuse:
        given = [f for f, v in (("--poses", args.poses is not None), ("--poses_c2w", args.poses_c2w), ("--fuse_voxel", args.fuse_voxel is not None),
                                ("--fuse_trunc", args.fuse_trunc is not None), ("--fuse_dims", args.fuse_dims is not None), ("--fuse_origin", args.fuse_origin is not None),
                                ("--fuse_min_weight", args.fuse_min_weight is not None), ("--fuse_max_weight", args.fuse_max_weight is not None)) if v]
        if given:
            raise SystemExit("md_rdm_amd.predict: --poses, --poses_c2w, --fuse_voxel, --fuse_trunc, --fuse_dims, --fuse_origin, --fuse_min_weight and --fuse_max_weight "
                             "need --fuse (got %s)" % " ".join(given))
        return None
    if not args.metric:
        raise SystemExit("md_rdm_amd.predict: --fuse needs --metric: a volume is made of depth in metres")
    if not (args.native or (args.synthetic and args.full_res)):
        raise SystemExit("md_rdm_amd.predict: --fuse needs the colours of the saved frame and its camera: --native for file inputs, --full_res for --synthetic "
                         "inputs (the frame is then the network input itself)")
    if args.poses is None:
        raise SystemExit("md_rdm_amd.predict: --fuse needs --poses FILE: one world-to-camera pose per input frame")
    for flag, v in (("--fuse_voxel", args.fuse_voxel), ("--fuse_trunc", args.fuse_trunc)):
        if v is not None and not (math.isfinite(v) and v > 0):
            raise SystemExit("md_rdm_amd.predict: %s must be finite and > 0 (got %r)" % (flag, v))
    if args.fuse_dims is not None and not (min(args.fuse_dims) > 0 and args.fuse_dims[0] * args.fuse_dims[1] * args.fuse_dims[2] <= 2 ** 31 - 1):
        raise SystemExit("md_rdm_amd.predict: --fuse_dims must be three positive integers with a product of at most 2^31 - 1 (got %r)" % (args.fuse_dims,))
    if args.fuse_origin is not None and not all(math.isfinite(v) for v in args.fuse_origin):
        raise SystemExit("md_rdm_amd.predict: --fuse_origin must be three finite values (got %r)" % (args.fuse_origin,))
    if args.fuse_min_weight is not None and math.isnan(args.fuse_min_weight):
        raise SystemExit("md_rdm_amd.predict: --fuse_min_weight must not be NaN")
    if args.fuse_max_weight is not None and not args.fuse_max_weight >= 1:
        raise SystemExit("md_rdm_amd.predict: --fuse_max_weight must be >= 1, the weight of one frame (got %r)" % args.fuse_max_weight)
    if (args.fuse_dims is None or args.fuse_origin is None) and args.max_depth is None:
        raise SystemExit("md_rdm_amd.predict: --fuse sizes its volume from the cameras' frusta up to --max_depth: give --max_depth, or --fuse_dims and --fuse_origin")
    poses = load_poses(args.poses)
    n_in = args.synthetic or len(args.inputs)
    if len(poses) != n_in:
        raise SystemExit("md_rdm_amd.predict: --poses takes one row per input frame (got %d rows for %d inputs)" % (len(poses), n_in))
    if args.poses_c2w:
        from .fuse import pose_inverse
        poses = pose_inverse(poses.reshape(-1, 3, 4)).reshape(-1, 12)
    return poses


def fuse_volume(args, poses, frames, intr_of, dev):
    """the ``fuse.Volume`` of --fuse: ``frames`` the distinct saved-frame shapes, ``intr_of(frame)`` their intrinsics.  Origin and dims are
    ``fuse.bounds``' over all the frames' frusta where they are not given; dims alone: the voxels from the given origin to that box's far corner."""
    import math
    from . import fuse
    from ._lib import RdmError
    voxel = args.fuse_voxel if args.fuse_voxel is not None else fuse.VOXEL
    origin, dims = args.fuse_origin, args.fuse_dims
    try:
        if origin is None or dims is None:
            boxes = [fuse.bounds(f, intr_of(f), poses.reshape(-1, 3, 4), args.max_depth, voxel) for f in frames]
            lo = [min(o[a] for o, _ in boxes) for a in range(3)]
            hi = [max(o[a] + (d[a] - 1) * voxel for o, d in boxes) for a in range(3)]
            origin = lo if origin is None else origin
            dims = [max(1, math.ceil((hi[a] - origin[a]) / voxel) + 1) for a in range(3)] if dims is None else dims
        return fuse.Volume(dims, origin, voxel, trunc=args.fuse_trunc, color=True, max_weight=args.fuse_max_weight if args.fuse_max_weight is not None else fuse.MAX_WEIGHT,
                           device=dev)
    except RdmError as e:
        raise SystemExit("md_rdm_amd.predict: --fuse: %s" % e)


def anchor_options(args):
    """--anchor* -> the ``anchor`` argument of predict_metric"""
    opts = {k: v for k, v in (("fit", args.anchor_fit), ("cell", args.anchor_cell), ("sigma", args.anchor_sigma), ("lam", args.anchor_lambda), ("reject", args.anchor_reject),
                              ("min_depth", args.min_depth), ("max_depth", args.max_depth)) if v is not None}
    opts["field"] = not args.anchor_no_field
    return opts


def load_anchor(path, unit):
    """float32 (H,W) metres: a .npy array as it is, a 16-bit greyscale PNG in steps of ``unit`` metres (one float64 product per pixel, rounded once)"""
    import numpy as np
    from . import viz
    if os.path.splitext(path)[1].lower() == ".npy":
        a = np.load(path)
        if a.ndim == 3 and a.shape[0] == 1:
            a = a[0]
        if a.ndim != 2 or a.dtype != np.float32:
            raise SystemExit(f"md_rdm_amd.predict: {path}: an anchor .npy must be a float32 HxW (or 1xHxW) frame in metres, got {a.dtype} {a.shape}")
        return np.ascontiguousarray(a)
    try:
        steps = viz.read_png16(path)
    except ValueError as e:
        raise SystemExit("md_rdm_amd.predict: %s" % e)
    return (steps.astype(np.float64) * unit).astype(np.float32)


def view_jobs(args):
    """[(file suffix, (3,4) pose)] of the views asked for"""
    import numpy as np
    from . import warp
    jobs = []
    if args.stereo is not None:
        jobs.append(("_right", warp.stereo_pose(args.stereo)))
    if args.view_pose is not None:
        jobs.append(("_view", np.asarray(args.view_pose, np.float64).reshape(3, 4)))
    return jobs


def depth_steps(d, unit):
    """float32 metres -> uint16 steps by the rule include/rdm_depth.h states for its depth_u16 plane, in the arithmetic it states it in: q = D / unit
    is ONE float64 division of the widened depth (csrc/depthout_dev.h's depth_quantise divides in float64 too), NaN -> 0, q >= 65535 -> 65535,
    otherwise rint(q), ties to even.  On the host: the library quantises only while it writes a frame (rdm_depth_frames from a log map,
    rdm_depth_refine from its filter) and has no entry point that quantises a finished float32 plane such as a warped one."""
    import numpy as np
    q = np.nan_to_num(np.asarray(d, np.float64) / unit, nan=0.0, posinf=65535.0)
    return np.rint(np.clip(q, 0.0, 65535.0)).astype(np.uint16)


def refine_options(args):
    """--refine* -> the ``refine`` argument of predict_metric"""
    if not args.refine:
        return None
    opts = {k: v for k, v in (("radius", args.refine_radius), ("step", args.refine_step), ("sigma_space", args.refine_sigma_space), ("sigma_color", args.refine_sigma_color))
            if v is not None}
    opts["fill"] = bool(args.refine_fill)
    return opts


def load_frame(path):
    """uint8 (H,W,3)"""
    import numpy as np
    ext = os.path.splitext(path)[1].lower()
    if ext == ".npy":
        a = np.load(path)
    elif ext == ".npz":
        with np.load(path) as z:
            a = z["rgb"] if "rgb" in z.files else z[z.files[0]]
    else:
        try:
            from PIL import Image
        except ImportError:
            raise SystemExit(f"md_rdm_amd.predict: {path}: reading image files needs Pillow, which is not installed; pass .npy / .npz uint8 HxWx3 frames instead")
        with Image.open(path) as im:
            a = np.asarray(im.convert("RGB"))
    if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8:
        raise SystemExit(f"md_rdm_amd.predict: {path}: need a uint8 HxWx3 frame, got {a.dtype} {a.shape}")
    return np.ascontiguousarray(a)


def main(argv=None):
    args = build_parser().parse_args(argv)
    if bool(args.synthetic) == bool(args.inputs):
        raise SystemExit("md_rdm_amd.predict: give input files or --synthetic N (not both)")
    if args.batch_size < 1:
        raise SystemExit("md_rdm_amd.predict: --batch_size must be positive")
    if args.ema and not args.checkpoint:
        raise SystemExit("md_rdm_amd.predict: --ema needs --checkpoint: the averaged weights are an entry of a checkpoint")
    check_png_args(args)
    check_metric_args(args)
    check_ply_args(args)
    check_refine_args(args)
    check_mesh_args(args)
    check_view_args(args)
    check_anchor_args(args)
    fuse_poses = check_fuse_args(args)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit(NO_GPU)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)

    from . import checkpoint, cloud, filler, mesh, viz, warp
    from .dataloaders import nyu
    from .network.RDM_Net import DepthEstimationNet
    model = DepthEstimationNet(relative_decoders=tuple(args.relative_decoders))
    if args.checkpoint:
        try:
            checkpoint.from_lightning(model, args.checkpoint, ema=args.ema)
        except checkpoint.NoAveragedWeights as e:                 # --ema on a checkpoint without averaged weights
            raise SystemExit("md_rdm_amd.predict: %s" % e.args[0])
    else:
        print("warning: no --checkpoint: using the deterministic hash-filled weights (filler.fill_state_dict) - the maps are not depth", flush=True)
        filler.fill_state_dict(model.state_dict())
    model = model.to(dev).eval().set_precision("bf16" if args.precision == 16 else "f32")
    size = tuple(args.size)
    os.makedirs(args.out, exist_ok=True)

    # (name, source) in order; batches are runs of inputs that share the raw frame size
    if args.synthetic:
        xs = filler.synthetic_batch(args.synthetic, size[0], size[1])[0]
        items = [("synthetic_%04d" % i, xs[i]) for i in range(args.synthetic)]
    else:
        items = [(os.path.splitext(os.path.basename(p))[0], load_frame(p)) for p in args.inputs]
    pre = nyu.NyuGpuPreprocessor(resize=500, output_size=size, device=dev)
    volume = None
    if args.fuse:                                                # the saved frames are raw frames (--native) or the network input (--synthetic --full_res)
        raw_intr = cloud.intrinsics_params(args.intrinsics if args.intrinsics is not None else args.camera or "nyu")
        volume = fuse_volume(args, fuse_poses, sorted({tuple(a.shape[:2]) for _, a in items}) if args.native else [size],
                             lambda f: raw_intr if args.native else cloud.intrinsics_in_view(raw_intr, (0.0, 0.0) + size, f), dev)
    seen, i = {}, 0
    while i < len(items):
        j = i + 1
        while j < len(items) and j - i < args.batch_size and items[j][1].shape == items[i][1].shape:
            j += 1
        batch = np.stack([a for _, a in items[i:j]])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if args.synthetic:
            x = torch.from_numpy(batch).to(dev)
            region = size
        else:
            rgb = torch.from_numpy(batch).to(dev)
            H, W = batch.shape[1:3]
            dummy = torch.zeros(len(batch), H, W, dtype=torch.float32, device=dev)        # the transform carries a depth plane; there is none here
            try:
                params = [nyu.test_params((H, W), size) for _ in range(len(batch))]
            except ValueError as e:
                raise SystemExit("md_rdm_amd.predict: %s (%dx%d frame): %s" % (items[i][0], H, W, e))
            x, _ = pre(rgb, dummy, params)
            region = (480, 640)
        if args.metric:
            frame = batch.shape[1:3] if args.native else region if args.full_res else (128, 128)
            anchored = {}
            if args.anchors is not None:
                frames = [load_anchor(p, args.anchor_unit or 1e-3) for p in args.anchors[i:j]]
                for p, a in zip(args.anchors[i:j], frames):
                    if a.shape != tuple(frame):
                        raise SystemExit("md_rdm_amd.predict: %s: the anchors are %dx%d, the saved frame is %dx%d" % ((p,) + a.shape + tuple(frame)))
                anchored = dict(anchors=torch.from_numpy(np.stack(frames)).to(dev), anchor=anchor_options(args))
            planes = model.predict_metric(x, frame, view=nyu.test_view(frame) if args.native else None, flip=args.flip, sid=args.sid or "nyu",
                                          offset=args.sid_offset or 0.0, unit=args.depth_unit or 1e-3, outside=args.outside or "zero",
                                          want=("f32", "u16") if args.png16 else ("f32",), refine=refine_options(args), guide=rgb if args.refine else None,
                                          **anchored)
            maps = planes["f32"].unsqueeze(1)
            steps = planes["u16"].cpu().numpy() if args.png16 else None
            views = view_jobs(args)
            if args.ply or views or args.fuse:
                intr = cloud.intrinsics_params(args.intrinsics if args.intrinsics is not None else args.camera or "nyu")
                if not args.native:                                  # the saved frame shows a rectangle of the raw frame (all of the network input for --synthetic)
                    intr = cloud.intrinsics_in_view(intr, (0.0, 0.0) + tuple(size) if args.synthetic else nyu.test_view(batch.shape[1:3]), frame)
            rendered = []
            if views or args.fuse:                                   # --synthetic --full_res: the frame is the network input, whose values in [0, 1) are the colours
                colours = rgb if args.native else (x.permute(0, 2, 3, 1) * 255.0).clamp(0.0, 255.0).to(torch.uint8).contiguous()
                if args.fuse:
                    volume.integrate(planes["f32"], intr, fuse_poses[i:j].reshape(-1, 3, 4), rgb=colours, min_depth=args.min_depth or 0.0,
                                     max_depth=args.max_depth if args.max_depth is not None else float("inf"))
                for suffix, pose in views:
                    r = warp.render(planes["f32"], intr, pose, rgb=colours, min_depth=args.min_depth or 0.0, max_depth=args.max_depth if args.max_depth is not None else float("inf"),
                                    splat=args.view_splat if args.view_splat is not None else warp.SPLAT, fill=args.view_fill if args.view_fill is not None else warp.FILL,
                                    want=("depth", "rgb") if args.png16 else ("rgb",))
                    rendered.append((suffix, r["rgb"].cpu().numpy(), depth_steps(r["depth"].cpu().numpy(), args.depth_unit or 1e-3) if args.png16 else None))
            if args.ply:
                ply_args = dict(rgb=rgb if args.native else None, normals=args.ply_normals, min_depth=args.min_depth or 0.0,
                                max_depth=args.max_depth if args.max_depth is not None else float("inf"), step=args.ply_step or 1)
                if args.mesh:
                    records, counts, tris, fcounts = mesh.depth_mesh(planes["f32"], intr, edge_ratio=args.mesh_edge_ratio if args.mesh_edge_ratio is not None else mesh.EDGE_RATIO,
                                                                     **ply_args)
                    face_counts = fcounts.cpu().tolist()
                else:
                    records, counts = cloud.point_cloud(planes["f32"], intr, **ply_args)
                ply_counts = counts.cpu().tolist()
        else:
            maps = model.predict(x, linear=args.linear, size=region if args.full_res else None, flip=args.flip)
        out = maps.cpu().numpy()
        dt = time.perf_counter() - t0
        if args.png:
            lo, hi = args.png_range if args.png_range is not None else (None, None)
            pngs = (viz.comparison_rows(x, None, maps, lo, hi) if args.png_with_input else viz.colorize(maps, lo, hi)).cpu().numpy()
        for n, ((name, _), m) in enumerate(zip(items[i:j], out)):
            k = seen.get(name, 0)
            seen[name] = k + 1
            stem = os.path.join(args.out, name + ("" if k == 0 else "_%d" % k))
            np.save(stem + ".npy", m)
            if args.png:
                viz.write_png(stem + ".png", pngs[n])
            if args.metric and args.png16:
                viz.write_png16(stem + "_depth.png", steps[n])
            for suffix, pics, dsteps in rendered if args.metric else ():
                viz.write_png(stem + suffix + ".png", pics[n])
                if dsteps is not None:
                    viz.write_png16(stem + suffix + "_depth.png", dsteps[n])
            if args.ply and args.mesh:
                mesh.write_ply(stem + ".ply", records[n], ply_counts[n], args.ply_normals, args.native, tris[n], face_counts[n])
            elif args.ply:
                cloud.write_ply(stem + ".ply", records[n], ply_counts[n], args.ply_normals, args.native)
        print("batch of %d: %.1f images/s" % (j - i, (j - i) / dt), flush=True)
        i = j
    if args.fuse:
        from . import fuse
        path = os.path.join(args.out, "fused.ply")
        n = volume.write_ply(path, normals=args.ply_normals, min_weight=args.fuse_min_weight if args.fuse_min_weight is not None else fuse.MIN_WEIGHT)
        print("fused %d frames into %d x %d x %d voxels of %g m: %d surface points in %s" % ((len(items),) + tuple(volume.dims) + (volume.voxel, n, path)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
