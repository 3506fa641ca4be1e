#!/usr/bin/env python3
"""One command line for the scripts of the package (the authors' roadmap item 3,
``recap_future_updates.md:8,14``: "a CLI that shows the user the various possibilities for the
parameters and the usages of the various scripts").  EXTENSION: the reference has two separate
argparse scripts (bbme.py:658-714, results.py:117-138); their flags are kept as they are.

    python gme_cli.py bbme    -p <video|frame dir> -fi 13 -bs 16 -sw 16 -sp 0     # bbme.py main
    python gme_cli.py results -v <name under resources/videos> -f 1 [--model quadratic] [--suggest]    # results.py main
    python gme_cli.py suggest -p <video|frame dir> [-fi 1] [-f 1]                 # parameter heuristics
    python gme_cli.py projective -p <video|frame dir> -fi 1 [-f 1]                # direct projective refinement of one pair
    python gme_cli.py stabilize -p <video|frame dir> -o OUTDIR [--estimator projective|affine] [--radius 15] [--neighbours 0]   # video stabilization
    python gme_cli.py mosaic -p <video|frame dir> -o OUTDIR [--estimator projective|affine] [--anchor 0] [--threshold 16] [--min-count 3] [--no-masks]   # background mosaic, moving-object masks
    python gme_cli.py subpel -p <video|frame dir> -fi 1 [-fd 1] [-bs 16] [-sw 16] [-sp 0] [-pn 0] [--levels 2] [-o OUTDIR]   # quarter-pel block matching of one pair
    python gme_cli.py hier -p <video|frame dir> -fi 1 [-fd 1] [-bs 16] [-cw 8] [-r 1] [-pn 0] [--levels 3] [--subpel 0|1|2] [-o OUTDIR]   # hierarchical block matching of one pair
    python gme_cli.py vbs -p <video|frame dir> -fi 1 [-fd 1] [-bs 16] [-sw 16] [-sp 0] [-pn 0] [--depth 2] [-r 1] [--penalty N] [--hier] [-o OUTDIR]   # variable-block-size motion of one pair
    python gme_cli.py bipred -p <video|frame dir> -fi 1 [-fd 1] [-bs 16] [-sw 16] [-sp 0] [-pn 0] [-r 1] [--rounds 1] [--penalty N] [-o OUTDIR]   # bidirectional prediction of one frame
    python gme_cli.py gmc -p <video|frame dir> -fi 1 [-fd 1] [-bs 16] [-sw 16] [-sp 0] [-pn 0] [--penalty N] [--estimator projective|affine] [-o OUTDIR]   # global motion compensation of one pair
    python gme_cli.py prop -p <video|frame dir> -fi 1 [-fd 1] [-bs 16] [-sw 16] [-sp 3] [-pn 0] [--rounds 2] [--steps 1] [--no-temporal] [--camera projective|affine|none] [--hier] [-o OUTDIR]   # vector propagation search of one pair
    python gme_cli.py retime -p <video|frame dir> -o OUTDIR (--rate-in 24 --rate-out 60 | --slow 4) [-bs 16] [-sw 16] [-pn 0] [--bias N]   # frame-rate conversion, slow motion
    python gme_cli.py retime -p <video|frame dir> -fi 0 --phase 1/3 [-fd 3] [-o OUTDIR]   # one frame at a phase between two frames
    python gme_cli.py interp -p <video|frame dir> -fi 2 [-fd 2] [-bs 16] [-sw 8] [-pn 0] [--bias N] [-o OUTDIR] [--upconvert]   # the frame between two frames; frame-rate doubling
    python gme_cli.py obmc -p <video|frame dir> -fi 1 [-fd 1] [-bs 16] [-sw 16] [-sp 0] [-pn 0] [--subpel 0|1|2] [--hier] [-o OUTDIR]   # overlapped block motion compensation of one pair
    python gme_cli.py denoise -p <video|frame dir> -o OUTDIR [-fd 1] [-bs 16] [-sw 8] [-sp 0] [-pn 0] [--radius 1] [--subpel 0|1|2] [--strength 24] [--noise SIGMA [--seed N]]   # motion-compensated temporal denoising of a clip
    python gme_cli.py info                                                       # searches, norms, models, device
"""
import argparse
import sys


def _models():
    import roadmap
    return roadmap.MODELS


def _parser():
    ap = argparse.ArgumentParser(prog="gme_cli.py", description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="command", required=True)
    b = sub.add_parser("bbme", help="motion field between two frames, plain and hierarchical (bbme.py:617-649)")
    b.add_argument("-p", "--video-path", dest="path", type=str, required=True, help="video file, frame directory, .npy or .y4m")
    b.add_argument("-fi", "--frame-index", dest="fi", type=int, required=True, help="index of the current frame (the previous one is fi - 3)")
    b.add_argument("-pn", "--p-norm", dest="pnorm", type=int, default=0, help="parsed and ignored, as upstream (the norm stays MSE)")
    b.add_argument("-bs", "--block-size", dest="block_size", type=int, default=12)
    b.add_argument("-sw", "--search-window", dest="search_window", type=int, default=8)
    b.add_argument("-sp", "--searching-procedure", dest="searching_procedure", type=int, default=1,
                   help="0: exhaustive, 1: three-step, 2: 2-D log, 3: diamond")
    r = sub.add_parser("results", help="global motion estimation + compensation + PSNR over a whole video (results.py:14-138)")
    r.add_argument("-v", "--video-name", dest="path", type=str, required=True, help="name under resources/videos (file or frame directory)")
    r.add_argument("-f", "--frame-distance", dest="fd", type=str, required=False)
    r.add_argument("--block-size", type=int, default=None, help="motion.BBME_BLOCK_SIZE for this run (the authors patched the constant by hand)")
    r.add_argument("--outlier-fraction", type=float, default=None, help="motion.MOTION_VECTOR_ERROR_THRESHOLD_PERCENTAGE for this run")
    r.add_argument("--model", choices=_models(), default="affine",
                   help="motion model fitted per level (roadmap.solve_model); affine is the reference")
    r.add_argument("--suggest", action="store_true",
                   help="pick block size and outlier fraction for this video with roadmap.suggest_parameters (middle pair); "
                        "explicit --block-size / --outlier-fraction win")
    s = sub.add_parser("suggest", help="heuristic block size / search window / outlier fraction for a frame pair (roadmap.suggest_parameters)")
    s.add_argument("-p", "--video-path", dest="path", type=str, required=True)
    s.add_argument("-fi", "--frame-index", dest="fi", type=int, default=1)
    s.add_argument("-f", "--frame-distance", dest="fd", type=int, default=1)
    j = sub.add_parser("projective", help="direct projective refinement of one frame pair (roadmap.refine_projective, DESIGN.md 7b)")
    j.add_argument("-p", "--video-path", dest="path", type=str, required=True, help="video file, frame directory, .npy or .y4m")
    j.add_argument("-fi", "--frame-index", dest="fi", type=int, required=True, help="index of the current frame")
    j.add_argument("-f", "--frame-distance", dest="fd", type=int, default=1)
    j.add_argument("--outlier-fraction", type=float, default=0.1)
    j.add_argument("--max-iters", type=int, default=10)
    st = sub.add_parser("stabilize", help="stabilize a whole video from its estimated camera path (stabilize.py, DESIGN.md 7c)")
    st.add_argument("-p", "--video-path", dest="path", type=str, required=True, help="video file, frame directory, .npy or .y4m")
    st.add_argument("-o", "--output", dest="outdir", type=str, required=True,
                    help="directory for stabilized/%%04d.png and stabilize.json")
    st.add_argument("--estimator", choices=("projective", "affine"), default="projective")
    st.add_argument("--radius", type=int, default=15, help="half-width of the Gaussian path filter, frames")
    st.add_argument("--sigma", type=float, default=None, help="its standard deviation (default radius / 3)")
    st.add_argument("--crop", type=_crop, default="auto", help="auto, or a fixed crop fraction in [0, 1)")
    st.add_argument("--max-crop", type=float, default=0.25, help="cap of the auto crop")
    st.add_argument("--border", choices=("constant", "replicate"), default="constant")
    st.add_argument("--fill", type=int, default=0, help="value of border pixels under --border constant")
    st.add_argument("--neighbours", type=int, default=0,
                    help="fill the border of each frame from this many frames a side (0 .. 8; crop auto then means 0)")
    mo =sub.add_parser("mosaic", help="background mosaic and moving-object masks from the estimated camera path (mosaic.py, DESIGN.md 7d)")
    mo.add_argument("-p", "--video-path", dest="path", type=str, required=True, help="video file, frame directory, .npy or .y4m")
    mo.add_argument("-o", "--output", dest="outdir", type=str, required=True,
                    help="directory for mosaic.png, masks/%%04d.png and mosaic.json")
    mo.add_argument("--estimator", choices=("projective", "affine"), default="projective")
    mo.add_argument("--anchor", type=int, default=0, help="the frame whose coordinates the canvas is laid out in")
    mo.add_argument("--threshold", type=int, default=16, help="mean residual of the 3x3 neighbourhood above which a pixel moves, grey levels")
    mo.add_argument("--min-count", dest="min_count", type=int, default=3, help="samples a sprite pixel needs before it predicts anything")
    mo.add_argument("--fill", type=int, default=0, help="value of sprite pixels no frame covers")
    mo.add_argument("--no-masks", dest="masks", action="store_false", help="build the mosaic only")
    sp = sub.add_parser("subpel", help="quarter-pel block matching of one frame pair: refine, compensate, report (subpel.py, DESIGN.md 7e)")
    sp.add_argument("-p", "--video-path", dest="path", type=str, required=True, help="video file, frame directory, .npy or .y4m")
    sp.add_argument("-fi", "--frame-index", dest="fi", type=int, required=True, help="index of the current frame")
    sp.add_argument("-fd", "--frame-distance", dest="fd", type=int, default=1)
    sp.add_argument("-bs", "--block-size", dest="block_size", type=int, default=16)
    sp.add_argument("-sw", "--search-window", dest="search_window", type=int, default=16)
    sp.add_argument("-sp", "--searching-procedure", dest="searching_procedure", type=int, default=0,
                    help="0: exhaustive, 1: three-step, 2: 2-D log, 3: diamond")
    sp.add_argument("-pn", "--p-norm", dest="pnorm", type=int, default=0, help="0: MAE, 1: MSE")
    sp.add_argument("--levels", type=int, default=2, help="0: integer, 1: half-pel, 2: quarter-pel")
    sp.add_argument("-o", "--output", dest="outdir", type=str, default=None, help="directory for subpel.json")
    hp = sub.add_parser("hier", help="hierarchical block matching of one frame pair: coarse-to-fine search, compensate, report (hier.py, DESIGN.md 7f)")
    hp.add_argument("-p", "--video-path", dest="path", type=str, required=True, help="video file, frame directory, .npy or .y4m")
    hp.add_argument("-fi", "--frame-index", dest="fi", type=int, required=True, help="index of the current frame")
    hp.add_argument("-fd", "--frame-distance", dest="fd", type=int, default=1)
    hp.add_argument("-bs", "--block-size", dest="block_size", type=int, default=16, help="at full resolution; halved per level")
    hp.add_argument("-cw", "--coarse-window", dest="coarse_window", type=int, default=8, help="+-pixels searched at the coarsest level (0 .. 8)")
    hp.add_argument("-r", "--radius", dest="radius", type=int, default=1, help="+-pixels searched around twice the parent vector below it (0 .. 3)")
    hp.add_argument("-pn", "--p-norm", dest="pnorm", type=int, default=0, help="0: MAE, 1: MSE")
    hp.add_argument("--levels", type=int, default=3, help="pyramid levels searched (1 .. 3)")
    hp.add_argument("--subpel", type=int, default=0, help="refine the field afterwards: 0 no, 1 half-pel, 2 quarter-pel")
    hp.add_argument("-o", "--output", dest="outdir", type=str, default=None, help="directory for hier.json")
    vp = sub.add_parser("vbs", help="variable-block-size motion of one frame pair: search, quadtree split and refine, both compensations (vbs.py, DESIGN.md 7g)")
    vp.add_argument("-p", "--video-path", dest="path", type=str, required=True, help="video file, frame directory, .npy or .y4m")
    vp.add_argument("-fi", "--frame-index", dest="fi", type=int, required=True, help="index of the current frame")
    vp.add_argument("-fd", "--frame-distance", dest="fd", type=int, default=1, help="the previous frame is fi - fd")
    vp.add_argument("-bs", "--block-size", dest="block_size", type=int, default=16, help="side of the root blocks")
    vp.add_argument("-sw", "--search-window", dest="search_window", type=int, default=16, help="search window (with --hier: the coarse window, 0 .. 8)")
    vp.add_argument("-sp", "--searching-procedure", dest="searching_procedure", type=int, default=0)
    vp.add_argument("-pn", "--pnorm-distance", dest="pnorm", type=int, default=0, help="0: MAE, 1: MSE")
    vp.add_argument("--depth", type=int, default=2, help="levels of the quadtree below the root (0 .. 2)")
    vp.add_argument("-r", "--radius", dest="radius", type=int, default=1, help="a child is searched within +-radius of its parent's vector (0 .. 3)")
    vp.add_argument("--penalty", type=int, default=None,
                    help="what a split must gain (0 .. 2^30); default: one grey level per pixel of the root, bs^2 for MAE and "
                         "16 bs^2 for MSE, a convention of this tool and not a tuned value")
    vp.add_argument("--hier", action="store_true", help="take the root field from the hierarchical search (three levels, radius 1)")
    vp.add_argument("-o", "--output", dest="outdir", type=str, default=None, help="directory for vbs.json")
    bp = sub.add_parser("bipred", help="bidirectional prediction of one frame from the frames on both sides of it: per block the past one, the next one or their average (bipred.py, DESIGN.md 7h)")
    bp.add_argument("-p", "--video-path", dest="path", type=str, required=True, help="video file, frame directory, .npy or .y4m")
    bp.add_argument("-fi", "--frame-index", dest="fi", type=int, required=True, help="index of the predicted frame")
    bp.add_argument("-fd", "--frame-distance", dest="fd", type=int, default=1, help="the references are fi - fd and fi + fd")
    bp.add_argument("-bs", "--block-size", dest="block_size", type=int, default=16, help="4 .. 64")
    bp.add_argument("-sw", "--search-window", dest="search_window", type=int, default=16)
    bp.add_argument("-sp", "--searching-procedure", dest="searching_procedure", type=int, default=0)
    bp.add_argument("-pn", "--pnorm-distance", dest="pnorm", type=int, default=0, help="0: MAE, 1: MSE")
    bp.add_argument("-r", "--radius", dest="radius", type=int, default=1, help="a pass tries one vector of the averaged pair within +-radius (0 .. 2)")
    bp.add_argument("--rounds", type=int, default=1, help="rounds of two passes, past vector then next vector (0 .. 2)")
    bp.add_argument("--penalty", type=int, default=None,
                    help="what the average must gain over a single reference (0 .. 2^30); default: a quarter grey level per pixel, "
                         "bs^2 / 4 for MAE and 4 bs^2 for MSE, a convention of this tool and not a tuned value")
    bp.add_argument("-o", "--output", dest="outdir", type=str, default=None, help="directory for bipred.json")
    gp = sub.add_parser("gmc", help="global motion compensation of one frame pair: per block the camera warp or the block's own vector (gmc.py, DESIGN.md 7i)")
    gp.add_argument("-p", "--video-path", dest="path", type=str, required=True, help="video file, frame directory, .npy or .y4m")
    gp.add_argument("-fi", "--frame-index", dest="fi", type=int, required=True, help="index of the predicted frame")
    gp.add_argument("-fd", "--frame-distance", dest="fd", type=int, default=1, help="the reference is fi - fd")
    gp.add_argument("-bs", "--block-size", dest="block_size", type=int, default=16, help="4 .. 64")
    gp.add_argument("-sw", "--search-window", dest="search_window", type=int, default=16)
    gp.add_argument("-sp", "--searching-procedure", dest="searching_procedure", type=int, default=0)
    gp.add_argument("-pn", "--pnorm-distance", dest="pnorm", type=int, default=0, help="0: MAE, 1: MSE")
    gp.add_argument("--penalty", type=int, default=None,
                    help="what the block's own vector must gain over the camera warp (0 .. 2^30); default: a quarter grey level per "
                         "pixel, bs^2 / 4 for MAE and 4 bs^2 for MSE, bipred's convention and not a tuned value")
    gp.add_argument("--estimator", choices=("projective", "affine"), default="projective",
                    help="the warp: the direct projective refinement, or the indirect affine estimate written as a warp")
    gp.add_argument("-o", "--output", dest="outdir", type=str, default=None, help="directory for gmc.json and modes.png")
    pp = sub.add_parser("prop", help="vector propagation search of one frame pair: neighbour, temporal and camera candidates on a prior field, refined by one pixel (propagate.py, DESIGN.md 7j)")
    pp.add_argument("-p", "--video-path", dest="path", type=str, required=True, help="video file, frame directory, .npy or .y4m")
    pp.add_argument("-fi", "--frame-index", dest="fi", type=int, required=True, help="index of the current frame")
    pp.add_argument("-fd", "--frame-distance", dest="fd", type=int, default=1, help="the previous frame is fi - fd; frame fi - 2 fd gives the temporal prior where it exists")
    pp.add_argument("-bs", "--block-size", dest="block_size", type=int, default=16, help="4 .. 64")
    pp.add_argument("-sw", "--search-window", dest="search_window", type=int, default=16, help="search window of the prior (with --hier: the coarse window, 0 .. 8)")
    pp.add_argument("-sp", "--searching-procedure", dest="searching_procedure", type=int, default=3, help="the search that makes the prior field")
    pp.add_argument("-pn", "--pnorm-distance", dest="pnorm", type=int, default=0, help="0: MAE, 1: MSE")
    pp.add_argument("--rounds", type=int, default=2, help="rounds, each on the field of the round before (1 .. 4)")
    pp.add_argument("--steps", type=int, default=1, help="refinement passes of one pixel per round (0 .. 4)")
    pp.add_argument("--no-temporal", dest="temporal", action="store_false", help="leave out the previous pair's vector")
    pp.add_argument("--camera", choices=("projective", "affine", "none"), default="projective",
                    help="the camera candidate: the direct projective refinement, the indirect affine estimate written as a warp, or none")
    pp.add_argument("--hier", action="store_true", help="take the prior field from the hierarchical search (three levels, radius 1)")
    pp.add_argument("-o", "--output", dest="outdir", type=str, default=None, help="directory for prop.json")
    ip = sub.add_parser("interp", help="motion-compensated frame interpolation: the frame halfway between two frames by a bilateral block search; frame-rate doubling of a clip (interp.py, DESIGN.md 7m)")
    ip.add_argument("-p", "--video-path", dest="path", type=str, required=True, help="video file, frame directory, .npy or .y4m")
    ip.add_argument("-fi", "--frame-index", dest="fi", type=int, required=True, help="index of the later frame of the pair")
    ip.add_argument("-fd", "--frame-distance", dest="fd", type=int, default=2,
                    help="the earlier frame is fi - fd; for an even distance frame fi - fd / 2 is the truth the result is compared with")
    ip.add_argument("-bs", "--block-size", dest="block_size", type=int, default=16, help="4 .. 64")
    ip.add_argument("-sw", "--search-window", dest="search_window", type=int, default=8, help="0 .. 8, per half step: content may move by twice as much between the two frames")
    ip.add_argument("-pn", "--pnorm-distance", dest="pnorm", type=int, default=0, help="0: MAE, 1: MSE")
    ip.add_argument("--bias", type=int, default=None,
                    help="cost of one unit of |vx| + |vy| (0 .. 2^16); default: bs^2 / 16 for MAE and bs^2 for MSE, a convention of this "
                         "tool and not a tuned value")
    ip.add_argument("-o", "--output", dest="outdir", type=str, default=None, help="directory for interp.json, interp.png and upconverted/%%04d.png")
    ip.add_argument("--upconvert", action="store_true", help="also double the frame rate of the whole clip into OUTDIR/upconverted/%%04d.png")
    rp = sub.add_parser("retime", help="frame interpolation at any phase: frame-rate conversion and slow motion of a clip, or one frame at a phase n/d between two frames (retime.py, DESIGN.md 7r)")
    rp.add_argument("-p", "--video-path", dest="path", type=str, required=True, help="video file, frame directory, .npy or .y4m")
    rp.add_argument("--rate-in", dest="rate_in", type=int, default=None, help="frames per second of the clip (with --rate-out)")
    rp.add_argument("--rate-out", dest="rate_out", type=int, default=None, help="frames per second wanted: 24 -> 60 makes the step 2/5")
    rp.add_argument("--slow", type=int, default=None, help="slow motion by this factor: the step 1/K")
    rp.add_argument("-fi", "--frame-index", dest="fi", type=int, default=None, help="one pair: index of the earlier frame (with --phase)")
    rp.add_argument("--phase", type=str, default=None, help="one pair: n/d, 0 < n/d < 1, d <= 64 once reduced")
    rp.add_argument("-fd", "--frame-distance", dest="fd", type=int, default=None,
                    help="one pair: the later frame is fi + fd (default: d of --phase, as written; then frame fi + n is the truth the result is compared with)")
    rp.add_argument("-bs", "--block-size", dest="block_size", type=int, default=16, help="4 .. 64")
    rp.add_argument("-sw", "--search-window", dest="search_window", type=int, default=16, help="0 .. 16: how far content may move between the two frames")
    rp.add_argument("-pn", "--pnorm-distance", dest="pnorm", type=int, default=0, help="0: MAE, 1: MSE")
    rp.add_argument("--bias", type=int, default=None,
                    help="cost of one unit of |Vx| + |Vy| (0 .. 2^16); default: bs^2 / 16 for MAE and bs^2 for MSE, a convention of this "
                         "tool and not a tuned value")
    rp.add_argument("-o", "--output", dest="outdir", type=str, default=None, help="directory for retime.json and retimed/%%04d.png (a clip) or retime.png (one pair)")
    op = sub.add_parser("obmc", help="overlapped block motion compensation of one frame pair: search, optional sub-pel refinement, the plain and the overlapped compensation (obmc.py, DESIGN.md 7o)")
    op.add_argument("-p", "--video-path", dest="path", type=str, required=True, help="video file, frame directory, .npy or .y4m")
    op.add_argument("-fi", "--frame-index", dest="fi", type=int, required=True, help="index of the current frame")
    op.add_argument("-fd", "--frame-distance", dest="fd", type=int, default=1, help="the previous frame is fi - fd")
    op.add_argument("-bs", "--block-size", dest="block_size", type=int, default=16, help="4 .. 64")
    op.add_argument("-sw", "--search-window", dest="search_window", type=int, default=16, help="search window (with --hier: the coarse window, 0 .. 8)")
    op.add_argument("-sp", "--searching-procedure", dest="searching_procedure", type=int, default=0,
                    help="0: exhaustive, 1: three-step, 2: 2-D log, 3: diamond")
    op.add_argument("-pn", "--pnorm-distance", dest="pnorm", type=int, default=0, help="0: MAE, 1: MSE")
    op.add_argument("--subpel", type=int, default=0, help="refine the field afterwards: 0 no, 1 half-pel, 2 quarter-pel")
    op.add_argument("--hier", action="store_true", help="take the field from the hierarchical search (three levels, radius 1)")
    op.add_argument("-o", "--output", dest="outdir", type=str, default=None, help="directory for obmc.json and obmc.png")
    dp = sub.add_parser("denoise", help="motion-compensated temporal denoising of a clip: every frame averaged with the overlapped predictions of it from its neighbours, gated per pixel (denoise.py, DESIGN.md 7p)")
    dp.add_argument("-p", "--video-path", dest="path", type=str, required=True, help="video file, frame directory, .npy or .y4m")
    dp.add_argument("-o", "--output", dest="outdir", type=str, required=True, help="directory for denoise.json and denoised/%%04d.png")
    dp.add_argument("-fd", "--frame-distance", dest="fd", type=int, default=1, help="the references of frame t are t -+ d fd, d = 1 .. radius")
    dp.add_argument("-bs", "--block-size", dest="block_size", type=int, default=16, help="4 .. 64")
    dp.add_argument("-sw", "--search-window", dest="search_window", type=int, default=8)
    dp.add_argument("-sp", "--searching-procedure", dest="searching_procedure", type=int, default=0,
                    help="0: exhaustive, 1: three-step, 2: 2-D log, 3: diamond")
    dp.add_argument("-pn", "--pnorm-distance", dest="pnorm", type=int, default=0, help="0: MAE, 1: MSE")
    dp.add_argument("--radius", type=int, default=1, help="1 .. 2: references on each side of a frame")
    dp.add_argument("--subpel", type=int, default=0, help="refine the fields: 0 no, 1 half-pel, 2 quarter-pel")
    dp.add_argument("--strength", type=int, default=24,
                    help="1 .. 64 grey levels: a prediction's weight reaches zero where the mean absolute difference over the 3 x 3 window "
                         "reaches it; the default is a convention of the tool and not a tuned value")
    dp.add_argument("--noise", type=float, default=None, help="add Gaussian noise of this sigma to the clip first and report PSNR against the clean clip")
    dp.add_argument("--seed", type=int, default=0, help="seed of --noise")
    sub.add_parser("info", help="list searches, norms, motion models and the device")
    return ap


def _crop(text):
    return text if text == "auto" else float(text)


def _stabilize(args):
    """Stabilized frames into OUTDIR/stabilized/%04d.png and the run's record into OUTDIR/stabilize.json."""
    import json
    import os
    import numpy as np
    import stabilize
    import utils
    frames = np.stack([np.asarray(f, dtype=np.uint8) for f in utils.get_video_frames(args.path)])
    out, res = stabilize.stabilize(frames, estimator=args.estimator, radius=args.radius, sigma=args.sigma, crop=args.crop,
                                   max_crop=args.max_crop, border=args.border, fill=args.fill, neighbours=args.neighbours)
    d = os.path.join(args.outdir, "stabilized")
    os.makedirs(d, exist_ok=True)
    for k, f in enumerate(out):
        utils.write_image(os.path.join(d, "%04d.png" % k), f)
    record = {"options": {"path": args.path, "estimator": args.estimator, "radius": args.radius, "sigma": args.sigma,
                          "crop": args.crop, "max_crop": args.max_crop, "border": args.border, "fill": args.fill},
              "frames": int(len(out)), "crop": res["crop"], "itf_before": res["itf_before"], "itf_after": res["itf_after"],
              "pair_params": res["h"].tolist(), "pair_flags": res["pair_flags"].tolist(), "W": res["W"].tolist(),
              "frame_flags": res["flags"].tolist(), "valid": res["valid"].tolist()}
    if args.neighbours:
        record["options"]["neighbours"] = args.neighbours
        record.update(neighbours=res["neighbours"], filled=res["filled"].tolist(), unfilled=res["unfilled"].tolist())
    with open(os.path.join(args.outdir, "stabilize.json"), "w") as f:
        json.dump(record, f, indent=1)
    print("{} frames of shape {}, crop {:.4f}".format(len(out), out.shape[1:], res["crop"]))
    print("itf before: {:.4f} dB".format(res["itf_before"]))
    print("itf after:  {:.4f} dB".format(res["itf_after"]))
    return res


def _mosaic(args):
    """The sprite into OUTDIR/mosaic.png, the masks (0 / 255) into OUTDIR/masks/%04d.png, the run's record into
    OUTDIR/mosaic.json."""
    import json
    import os
    import numpy as np
    import mosaic
    import utils
    frames = np.stack([np.asarray(f, dtype=np.uint8) for f in utils.get_video_frames(args.path)])
    sprite, masks, res = mosaic.mosaic(frames, estimator=args.estimator, anchor=args.anchor, threshold=args.threshold,
                                       min_count=args.min_count, fill=args.fill, masks=args.masks)
    os.makedirs(args.outdir, exist_ok=True)
    utils.write_image(os.path.join(args.outdir, "mosaic.png"), sprite)
    if masks is not None:
        d = os.path.join(args.outdir, "masks")
        os.makedirs(d, exist_ok=True)
        for k, m in enumerate(masks):
            utils.write_image(os.path.join(d, "%04d.png" % k), m * np.uint8(255))
    record = {"options": {"path": args.path, "estimator": args.estimator, "anchor": args.anchor, "threshold": args.threshold,
                          "min_count": args.min_count, "fill": args.fill, "masks": bool(args.masks)},
              "frames": int(len(frames)), "origin": [res["ox"], res["oy"]], "size": [res["Hc"], res["Wc"]],
              "frame_flags": res["flags"].tolist(), "pair_params": res["h"].tolist(), "pair_flags": res["pair_flags"].tolist(),
              "known": res["known"].tolist() if masks is not None else None,
              "moving": res["moving"].tolist() if masks is not None else None}
    with open(os.path.join(args.outdir, "mosaic.json"), "w") as f:
        json.dump(record, f, indent=1)
    print("{} frames of shape {}: canvas {} x {} at origin ({}, {})".format(len(frames), frames.shape[1:], res["Hc"], res["Wc"],
                                                                          res["ox"], res["oy"]))
    print("covered: {:.2f} % of the canvas".format(100.0 * float(np.mean(res["count"] > 0))))
    if masks is not None:
        print("moving: {:.2f} % of the known pixels".format(100.0 * float(res["moving"].sum()) / max(1, int(res["known"].sum()))))
    return res


def _subpel(args):
    """Median vector, share of blocks moved off the integer vector and the PSNR of both compensations of one pair; the same
    record into OUTDIR/subpel.json."""
    import json
    import os
    import subpel
    import utils
    frames = utils.get_video_frames(args.path)
    if not args.fd <= args.fi < len(frames) or args.fd < 1:
        raise IndexError("frames %d and %d of %d" % (args.fi - args.fd, args.fi, len(frames)))
    res = subpel.report(frames[args.fi - args.fd], frames[args.fi], args.block_size, args.search_window, args.searching_procedure,
                        args.pnorm, args.levels)
    record = {"options": {"path": args.path, "frame_index": args.fi, "frame_distance": args.fd, "block_size": args.block_size,
                          "search_window": args.search_window, "searching_procedure": args.searching_procedure,
                          "pnorm": args.pnorm, "levels": args.levels},
              "shape": list(res["mf"].shape[:2])}
    record.update({k: res[k] for k in ("median_vector", "moved_share", "sse_integer", "sse_qpel", "psnr_integer", "psnr_qpel",
                                       "psnr_gain")})
    print("frames {} -> {}: {} x {} blocks of {}".format(args.fi - args.fd, args.fi, record["shape"][0], record["shape"][1],
                                                         args.block_size))
    print("median vector: ({:.2f}, {:.2f}) px".format(*record["median_vector"]))
    print("moved off the integer vector: {:.2f} % of the blocks".format(100.0 * record["moved_share"]))
    print("psnr integer:     {:.4f} dB".format(record["psnr_integer"]))
    print("psnr quarter-pel: {:.4f} dB  (gain {:+.4f} dB)".format(record["psnr_qpel"], record["psnr_gain"]))
    if args.outdir:
        os.makedirs(args.outdir, exist_ok=True)
        with open(os.path.join(args.outdir, "subpel.json"), "w") as f:
            json.dump(record, f, indent=1)
    return res


def _vbs(args):
    """Share of the roots split, leaves per depth and the PSNR of the root-field and the leaf-field compensation of one pair;
    the same record into OUTDIR/vbs.json."""
    import json
    import os
    import utils
    import vbs
    frames = utils.get_video_frames(args.path)
    if not args.fd <= args.fi < len(frames) or args.fd < 1:
        raise IndexError("frames %d and %d of %d" % (args.fi - args.fd, args.fi, len(frames)))
    if args.hier:
        args.search_window = min(args.search_window, 8)
    res = vbs.report(frames[args.fi - args.fd], frames[args.fi], args.block_size, args.search_window, args.searching_procedure,
                     args.pnorm, args.depth, args.radius, args.penalty, args.hier)
    record = {"options": {"path": args.path, "frame_index": args.fi, "frame_distance": args.fd, "block_size": args.block_size,
                          "search_window": args.search_window, "searching_procedure": args.searching_procedure,
                          "pnorm": args.pnorm, "depth": args.depth, "radius": args.radius, "penalty": res["penalty"],
                          "hier": bool(args.hier)},
              "shape": list(res["mf"].shape[:2])}
    record.update({k: res[k] for k in ("split_share", "leaves", "sse_root", "sse_leaf", "psnr_root", "psnr_leaf", "psnr_gain")})
    print("frames {} -> {}: {} x {} roots of {}, depth {}, radius {}, penalty {}".format(
        args.fi - args.fd, args.fi, record["shape"][0], record["shape"][1], args.block_size, args.depth, args.radius, res["penalty"]))
    print("roots split: {:.2f} %".format(100.0 * record["split_share"]))
    print("leaves per depth: " + ", ".join("{} of {}".format(n, args.block_size >> d) for d, n in enumerate(record["leaves"])))
    print("psnr root field: {:.4f} dB".format(record["psnr_root"]))
    print("psnr leaf field: {:.4f} dB  (gain {:+.4f} dB)".format(record["psnr_leaf"], record["psnr_gain"]))
    if args.outdir:
        os.makedirs(args.outdir, exist_ok=True)
        with open(os.path.join(args.outdir, "vbs.json"), "w") as f:
            json.dump(record, f, indent=1)
    return res


def _bipred(args):
    """Mode shares, the share of refined blocks and the PSNR of the past-only, the next-only and the chosen prediction of one
    frame; the same record into OUTDIR/bipred.json."""
    import json
    import os
    import bipred
    import utils
    frames = utils.get_video_frames(args.path)
    if args.fd < 1 or not args.fd <= args.fi < len(frames) - args.fd:
        raise IndexError("frames %d, %d and %d of %d" % (args.fi - args.fd, args.fi, args.fi + args.fd, len(frames)))
    res = bipred.report(frames[args.fi - args.fd], frames[args.fi], frames[args.fi + args.fd], args.block_size, args.search_window,
                        args.searching_procedure, args.pnorm, args.radius, args.rounds, args.penalty)
    record = {"options": {"path": args.path, "frame_index": args.fi, "frame_distance": args.fd, "block_size": args.block_size,
                          "search_window": args.search_window, "searching_procedure": args.searching_procedure,
                          "pnorm": args.pnorm, "radius": args.radius, "rounds": args.rounds, "penalty": res["penalty"]},
              "shape": list(res["mode"].shape)}
    record.update({k: res[k] for k in ("mode_share", "refined_share", "sse_past", "sse_next", "sse_chosen", "psnr_past", "psnr_next",
                                       "psnr_chosen")})
    print("frame {} from {} and {}: {} x {} blocks of {}, radius {}, rounds {}, penalty {}".format(
        args.fi, args.fi - args.fd, args.fi + args.fd, record["shape"][0], record["shape"][1], args.block_size, args.radius, args.rounds,
        res["penalty"]))
    print("modes: past {:.2f} %, next {:.2f} %, average {:.2f} %, none {:.2f} %".format(*(100.0 * v for v in record["mode_share"])))
    print("refined blocks: {:.2f} %".format(100.0 * record["refined_share"]))
    print("psnr past only: {:.4f} dB".format(record["psnr_past"]))
    print("psnr next only: {:.4f} dB".format(record["psnr_next"]))
    print("psnr chosen:    {:.4f} dB".format(record["psnr_chosen"]))
    if args.outdir:
        os.makedirs(args.outdir, exist_ok=True)
        with open(os.path.join(args.outdir, "bipred.json"), "w") as f:
            json.dump(record, f, indent=1)
    return res


def _interp(args):
    """The bias, the median vector and the share of non-zero vectors of one pair and, for an even frame distance, the PSNR of the
    interpolated frame and of the plain average against the true middle frame; the same record into OUTDIR/interp.json, the
    frame into OUTDIR/interp.png and, with --upconvert, the clip at twice the frame rate into OUTDIR/upconverted/%04d.png."""
    import json
    import os
    import numpy as np
    import interp
    import utils
    frames = utils.get_video_frames(args.path)
    if args.fd < 1 or not args.fd <= args.fi < len(frames):
        raise IndexError("frames %d and %d of %d" % (args.fi - args.fd, args.fi, len(frames)))
    truth = frames[args.fi - args.fd // 2] if args.fd % 2 == 0 else None
    res = interp.report(frames[args.fi - args.fd], frames[args.fi], truth, args.block_size, args.search_window, args.pnorm, args.bias)
    record = {"options": {"path": args.path, "frame_index": args.fi, "frame_distance": args.fd, "block_size": args.block_size,
                          "search_window": args.search_window, "pnorm": args.pnorm % 2, "bias": res["bias"]},
              "shape": list(res["mv"].shape[:2])}
    record.update({k: res[k] for k in ("median_vector", "nonzero_share", "sse_interp", "sse_average", "psnr_interp", "psnr_average") if k in res})
    print("the frame between {} and {}: {} x {} blocks of {}, window {}, bias {}".format(
        args.fi - args.fd, args.fi, record["shape"][0], record["shape"][1], args.block_size, args.search_window, res["bias"]))
    print("median vector: ({:g}, {:g})".format(*record["median_vector"]))
    print("non-zero vectors: {:.2f} %".format(100.0 * record["nonzero_share"]))
    if truth is not None:
        print("psnr interpolation: {:.4f} dB".format(record["psnr_interp"]))
        print("psnr plain average: {:.4f} dB".format(record["psnr_average"]))
    if args.outdir:
        os.makedirs(args.outdir, exist_ok=True)
        with open(os.path.join(args.outdir, "interp.json"), "w") as f:
            json.dump(record, f, indent=1)
        utils.write_image(os.path.join(args.outdir, "interp.png"), res["frame"])
        if args.upconvert:
            d = os.path.join(args.outdir, "upconverted")
            os.makedirs(d, exist_ok=True)
            clip = interp.upconvert(np.stack([np.asarray(f) for f in frames]), args.block_size, args.search_window, args.pnorm, args.bias)
            for k, f in enumerate(clip):
                utils.write_image(os.path.join(d, "%04d.png" % k), f)
            res["upconverted"] = clip
            print("up-converted: {} frames into {}".format(len(clip), d))
    return res


def _retime(args):
    """A clip (--rate-in / --rate-out or --slow): the schedule and, per made frame, the median vector and the share of non-zero
    vectors, into OUTDIR/retime.json, the frames into OUTDIR/retimed/%04d.png.  One pair (-fi, --phase n/d): the same figures
    and, where the later frame is d frames on, the PSNR of the made frame and of the plain cross-fade against frame fi + n; the
    record into OUTDIR/retime.json and the frame into OUTDIR/retime.png."""
    import json
    import os
    import numpy as np
    import retime
    import utils
    frames = utils.get_video_frames(args.path)
    options = {"path": args.path, "block_size": args.block_size, "search_window": args.search_window, "pnorm": args.pnorm % 2}
    if args.phase is not None:
        if args.fi is None:
            raise ValueError("--phase needs -fi, the index of the earlier frame")
        n, d = (int(t) for t in args.phase.split("/"))
        fd = d if args.fd is None else args.fd
        if fd < 1 or not 0 <= args.fi < args.fi + fd < len(frames):
            raise IndexError("frames %d and %d of %d" % (args.fi, args.fi + fd, len(frames)))
        truth = frames[args.fi + n] if fd == d and 0 < n < d else None
        res = retime.report(frames[args.fi], frames[args.fi + fd], n, d, truth, args.block_size, args.search_window, args.pnorm, args.bias)
        options.update(frame_index=args.fi, frame_distance=fd, phase=res["phase"], bias=res["bias"])
        record = {"options": options, "shape": list(res["mv"].shape[:2])}
        record.update({k: res[k] for k in ("median_vector", "nonzero_share", "sse_retime", "sse_crossfade", "psnr_retime", "psnr_crossfade") if k in res})
        print("the frame at phase {}/{} between {} and {}: {} x {} blocks of {}, window {}, bias {}".format(
            res["phase"][0], res["phase"][1], args.fi, args.fi + fd, record["shape"][0], record["shape"][1], args.block_size,
            args.search_window, res["bias"]))
        print("median vector: ({:g}, {:g})".format(*record["median_vector"]))
        print("non-zero vectors: {:.2f} %".format(100.0 * record["nonzero_share"]))
        if truth is not None:
            print("psnr retimed: {:.4f} dB".format(record["psnr_retime"]))
            print("psnr plain cross-fade: {:.4f} dB".format(record["psnr_crossfade"]))
        if args.outdir:
            os.makedirs(args.outdir, exist_ok=True)
            with open(os.path.join(args.outdir, "retime.json"), "w") as f:
                json.dump(record, f, indent=1)
            utils.write_image(os.path.join(args.outdir, "retime.png"), res["frame"])
        return res
    if args.slow is not None:
        if args.slow < 1:
            raise ValueError("--slow %d" % args.slow)
        step = (1, args.slow)
    elif args.rate_in is not None and args.rate_out is not None:
        step = retime.rate_step(args.rate_in, args.rate_out)
    else:
        raise ValueError("retime wants --rate-in and --rate-out, --slow, or -fi with --phase")
    if not args.outdir:
        raise ValueError("retime of a clip wants -o OUTDIR")
    clip = np.stack([np.asarray(f) for f in frames])
    rows = retime.schedule(len(clip), *step)
    made, mv, _, _ = retime.retime_clip(clip, step, args.block_size, args.search_window, args.pnorm, args.bias)
    bias = retime.default_bias(args.block_size, args.pnorm % 2) if args.bias is None else args.bias
    options.update(bias=bias)
    H, W = clip.shape[1:]
    per_frame = [{"copy_of": int(k)} if n == 0 else dict(retime.summary(mv[m], H, W), pair=[int(k), int(k) + 1], phase=[int(n), int(d)])
                 for m, (k, n, d) in enumerate(rows)]
    record = {"options": options, "step": list(step), "schedule": rows.tolist(), "frames": per_frame, "shape": list(mv.shape[1:3])}
    print("step {}/{}: {} frames from {}, {} x {} blocks of {}, window {}, bias {}".format(
        step[0], step[1], len(made), len(clip), record["shape"][0], record["shape"][1], args.block_size, args.search_window, bias))
    d = os.path.join(args.outdir, "retimed")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(args.outdir, "retime.json"), "w") as f:
        json.dump(record, f, indent=1)
    for m, f in enumerate(made):
        utils.write_image(os.path.join(d, "%04d.png" % m), f)
    return {"frames": made, "mv": mv, "schedule": rows, "record": record}


def _obmc(args):
    """The PSNR of the plain and of the overlapped compensation of one pair, by the integer field and, with --subpel above 0, by the
    refined field; the same record into OUTDIR/obmc.json and the overlapped compensation by the finest field into OUTDIR/obmc.png."""
    import json
    import os
    import obmc
    import utils
    frames = utils.get_video_frames(args.path)
    if not args.fd <= args.fi < len(frames) or args.fd < 1:
        raise IndexError("frames %d and %d of %d" % (args.fi - args.fd, args.fi, len(frames)))
    if args.hier:
        args.search_window = min(args.search_window, 8)
    res = obmc.report(frames[args.fi - args.fd], frames[args.fi], args.block_size, args.search_window, args.searching_procedure,
                      args.pnorm, args.subpel, args.hier)
    record = {"options": {"path": args.path, "frame_index": args.fi, "frame_distance": args.fd, "block_size": args.block_size,
                          "search_window": args.search_window, "searching_procedure": args.searching_procedure,
                          "pnorm": args.pnorm, "subpel": args.subpel, "hier": bool(args.hier)},
              "shape": list(res["mf"].shape[:2])}
    print("frames {} -> {}: {} x {} blocks of {}".format(args.fi - args.fd, args.fi, record["shape"][0], record["shape"][1],
                                                         args.block_size))
    for key, name in (("integer", "integer field"), ("qpel", "refined field")):
        if key in res:
            record[key] = res[key]
            print("psnr {}: plain {:.4f} dB, overlapped {:.4f} dB  (gain {:+.4f} dB)".format(
                name, res[key]["psnr_plain"], res[key]["psnr_obmc"], res[key]["psnr_gain"]))
    if args.outdir:
        os.makedirs(args.outdir, exist_ok=True)
        with open(os.path.join(args.outdir, "obmc.json"), "w") as f:
            json.dump(record, f, indent=1)
        utils.write_image(os.path.join(args.outdir, "obmc.png"), res["frame"])
    return res


def _denoise(args):
    """The filtered clip into OUTDIR/denoised/%04d.png and the record into OUTDIR/denoise.json: per frame the squared difference
    to the input, and with --noise (seeded Gaussian noise added to the clip first) the squared errors and the PSNR of the noisy and
    of the filtered clip against the clean one."""
    import json
    import os
    import numpy as np
    import denoise
    import utils
    frames = np.stack([np.ascontiguousarray(f) for f in utils.get_video_frames(args.path)])
    clean = None
    if args.noise is not None:
        clean = frames
        rng = np.random.default_rng(args.seed)
        frames = np.clip(np.rint(clean + rng.normal(scale=args.noise, size=clean.shape)), 0, 255).astype(np.uint8)
    res = denoise.report(frames, clean, frame_distance=args.fd, block_size=args.block_size, search_window=args.search_window,
                         searching_procedure=args.searching_procedure, pnorm_distance=args.pnorm, radius=args.radius, levels=args.subpel,
                         strength=args.strength)
    record = {"options": {"path": args.path, "frame_distance": args.fd, "block_size": args.block_size, "search_window": args.search_window,
                          "searching_procedure": args.searching_procedure, "pnorm": args.pnorm, "radius": args.radius,
                          "subpel": args.subpel, "strength": args.strength, "noise": args.noise, "seed": args.seed},
              "frames": len(frames), "shape": list(frames.shape[1:])}
    record.update({k: v for k, v in res.items() if k != "frames"})
    print("{} frames of {} x {}: strength {}, radius {}, changed by {} in all".format(len(frames), frames.shape[1], frames.shape[2],
                                                                                    args.strength, args.radius, sum(res["change"])))
    if clean is not None:
        print("psnr against the clean clip: noisy {:.4f} dB, filtered {:.4f} dB  (gain {:+.4f} dB)".format(
            res["psnr_noisy"], res["psnr_filtered"], res["psnr_filtered"] - res["psnr_noisy"]))
    os.makedirs(os.path.join(args.outdir, "denoised"), exist_ok=True)
    with open(os.path.join(args.outdir, "denoise.json"), "w") as f:
        json.dump(record, f, indent=1)
    for k, made in enumerate(res["frames"]):
        utils.write_image(os.path.join(args.outdir, "denoised", "%04d.png" % k), made)
    res["noisy"] = frames
    return res


def _gmc(args):
    """The penalty, the mode shares and the PSNR of the global-only, the local-only and the chosen prediction of one frame; the
    same record into OUTDIR/gmc.json and the mode map (0 / 128 / 255 per block, scaled up to the frame) into OUTDIR/modes.png."""
    import json
    import os
    import numpy as np
    import gmc
    import motion
    import roadmap
    import utils
    frames = utils.get_video_frames(args.path)
    if not args.fd <= args.fi < len(frames) or args.fd < 1:
        raise IndexError("frames %d and %d of %d" % (args.fi - args.fd, args.fi, len(frames)))
    ref, cur = frames[args.fi - args.fd], frames[args.fi]
    if args.estimator == "affine":
        h = roadmap.affine_to_projective(roadmap.global_motion_estimation(ref, cur), int(motion.BBME_BLOCK_SIZE))
    else:
        h = roadmap.refine_projective(ref, cur)[0]
    res = gmc.report(ref, cur, h, args.block_size, args.search_window, args.searching_procedure, args.pnorm, args.penalty)
    record = {"options": {"path": args.path, "frame_index": args.fi, "frame_distance": args.fd, "block_size": args.block_size,
                          "search_window": args.search_window, "searching_procedure": args.searching_procedure,
                          "pnorm": args.pnorm, "penalty": res["penalty"], "estimator": args.estimator},
              "shape": list(res["mode"].shape), "h": [float(v) for v in res["h"]], "usable": res["usable"]}
    record.update({k: res[k] for k in ("mode_share", "sse_global", "sse_local", "sse_chosen", "psnr_global", "psnr_local", "psnr_chosen")})
    print("frame {} from {}: {} x {} blocks of {}, {} warp{}, penalty {}".format(
        args.fi, args.fi - args.fd, record["shape"][0], record["shape"][1], args.block_size, args.estimator,
        "" if res["usable"] else " (unusable)", res["penalty"]))
    print("modes: global {:.2f} %, local {:.2f} %, none {:.2f} %".format(*(100.0 * v for v in record["mode_share"])))
    print("psnr global only: {:.4f} dB".format(record["psnr_global"]))
    print("psnr local only:  {:.4f} dB".format(record["psnr_local"]))
    print("psnr chosen:      {:.4f} dB".format(record["psnr_chosen"]))
    if args.outdir:
        os.makedirs(args.outdir, exist_ok=True)
        with open(os.path.join(args.outdir, "gmc.json"), "w") as f:
            json.dump(record, f, indent=1)
        grey = np.array([0, 128, 255], np.uint8)[res["mode"]]
        H, W = cur.shape
        big = np.zeros((H, W), np.uint8)
        tiles = np.kron(grey, np.ones((args.block_size, args.block_size), np.uint8))
        big[:tiles.shape[0], :tiles.shape[1]] = tiles
        utils.write_image(os.path.join(args.outdir, "modes.png"), big)
    return res


def _prop(args):
    """The share of blocks whose vector changed, the share per source class, the mean block cost and the PSNR of the integer
    compensation before and after the propagation of one pair; the same record into OUTDIR/prop.json."""
    import json
    import os
    import propagate
    import utils
    frames = utils.get_video_frames(args.path)
    if not args.fd <= args.fi < len(frames) or args.fd < 1:
        raise IndexError("frames %d and %d of %d" % (args.fi - args.fd, args.fi, len(frames)))
    if args.hier:
        args.search_window = min(args.search_window, 8)
    first = args.fi - 2 * args.fd if args.fi >= 2 * args.fd else args.fi - args.fd      # the pair before, for the temporal prior
    res = propagate.report([frames[k] for k in range(first, args.fi + 1, args.fd)], args.block_size, args.search_window,
                           args.searching_procedure, args.pnorm, args.rounds, args.steps, args.temporal, args.camera, args.hier, 1)
    record = {"options": {"path": args.path, "frame_index": args.fi, "frame_distance": args.fd, "block_size": args.block_size,
                          "search_window": args.search_window, "searching_procedure": args.searching_procedure, "pnorm": args.pnorm,
                          "rounds": args.rounds, "steps": args.steps, "temporal": res["temporal"], "camera": args.camera,
                          "hier": bool(args.hier)},
              "shape": list(res["mf"].shape[:2]), "h": None if res["h"] is None else [float(v) for v in res["h"]],
              "camera_field": res["g"] is not None}
    record.update({k: res[k] for k in ("changed_share", "source_share", "moved_share", "mean_cost_prior", "mean_cost_prop", "sse_prior",
                                       "sse_prop", "psnr_prior", "psnr_prop")})
    print("frames {} -> {}: {} x {} blocks of {}, rounds {}, steps {}, temporal prior {}, camera {}{}".format(
        args.fi - args.fd, args.fi, record["shape"][0], record["shape"][1], args.block_size, args.rounds, args.steps,
        "yes" if res["temporal"] else "no", args.camera, "" if res["g"] is not None or args.camera == "none" else " (no field)"))
    print("vectors changed: {:.2f} %".format(100.0 * record["changed_share"]))
    print("sources: " + ", ".join("{} {:.2f} %".format(k, 100.0 * v) for k, v in record["source_share"].items())
          + "; moved {:.2f} %".format(100.0 * record["moved_share"]))
    print("mean block cost: prior {:.2f}, propagated {:.2f}".format(record["mean_cost_prior"], record["mean_cost_prop"]))
    print("psnr prior field:      {:.4f} dB".format(record["psnr_prior"]))
    print("psnr propagated field: {:.4f} dB".format(record["psnr_prop"]))
    if args.outdir:
        os.makedirs(args.outdir, exist_ok=True)
        with open(os.path.join(args.outdir, "prop.json"), "w") as f:
            json.dump(record, f, indent=1)
    return res


def _hier(args):
    """Reach, median vector and PSNR of the compensation of one pair under the hierarchical search (with --subpel also the
    PSNR of the quarter-pel compensation of the refined field); the same record into OUTDIR/hier.json."""
    import json
    import os
    import hier
    import utils
    frames = utils.get_video_frames(args.path)
    if not args.fd <= args.fi < len(frames) or args.fd < 1:
        raise IndexError("frames %d and %d of %d" % (args.fi - args.fd, args.fi, len(frames)))
    prev, cur = frames[args.fi - args.fd], frames[args.fi]
    res = hier.report(prev, cur, args.block_size, args.coarse_window, args.radius, args.pnorm, args.levels)
    record = {"options": {"path": args.path, "frame_index": args.fi, "frame_distance": args.fd, "block_size": args.block_size,
                          "coarse_window": args.coarse_window, "radius": args.radius, "pnorm": args.pnorm, "levels": args.levels,
                          "subpel": args.subpel},
              "shape": list(res["field"].shape[:2])}
    record.update({k: res[k] for k in ("reach", "median_vector", "sse", "psnr")})
    print("frames {} -> {}: {} x {} blocks of {}".format(args.fi - args.fd, args.fi, record["shape"][0], record["shape"][1],
                                                         args.block_size))
    print("reach: +-{} px".format(record["reach"]))
    print("median vector: ({:.2f}, {:.2f}) px".format(*record["median_vector"]))
    print("psnr: {:.4f} dB".format(record["psnr"]))
    if args.subpel:
        import _gme_native
        import motion
        import subpel
        seq = motion._pair_sequence(prev, cur)
        seq.hier(1, args.block_size, args.coarse_window, args.radius, args.pnorm % 2, args.levels)
        seq.subpel(1, args.block_size, args.pnorm % 2, args.subpel)
        res["qfield"], res["qcost"] = (a[0] for a in seq.read_qmv())
        record["sse_qpel"] = int(seq.compensate_qpel(1, args.block_size)[0]) if res["field"].size else record["sse"]
        record["psnr_qpel"] = subpel.psnr(record["sse_qpel"], *_gme_native.as_frame(prev).shape)
        print("psnr quarter-pel: {:.4f} dB".format(record["psnr_qpel"]))
    if args.outdir:
        os.makedirs(args.outdir, exist_ok=True)
        with open(os.path.join(args.outdir, "hier.json"), "w") as f:
            json.dump(record, f, indent=1)
    return res


def _projective(args):
    """h, flags and the PSNR of the block-affine and of the projective compensation of one pair."""
    import numpy as np
    import _gme_native
    import motion
    import roadmap
    import sequence
    import utils
    frames = utils.get_video_frames(args.path)
    prev, cur = _gme_native.as_frame(frames[args.fi - args.fd]), _gme_native.as_frame(frames[args.fi])
    seq = motion._pair_sequence(prev, cur)
    bs = int(motion.BBME_BLOCK_SIZE)
    affine, sse_affine = roadmap.estimate_blocking(seq, 1, compensate=True)
    h, flags = roadmap.refine_sequence(seq, 1, roadmap.affine_to_projective(affine, bs), args.outlier_fraction, args.max_iters)
    sse_proj = seq.compensate_projective(1, h)
    psnr = sequence.psnr_from_sse(np.concatenate([sse_affine, sse_proj]), *prev.shape)
    print("frames {} -> {} of shape {}".format(args.fi - args.fd, args.fi, prev.shape))
    print("h: {}".format(" ".join("%.9g" % x for x in h[0])))
    print("flags: {}".format(int(flags[0])))
    print("psnr block-affine: {:.4f} dB".format(psnr[0]))
    print("psnr projective:   {:.4f} dB".format(psnr[1]))
    return {"h": h[0], "flags": int(flags[0]), "psnr_affine": float(psnr[0]), "psnr_projective": float(psnr[1])}


def main(argv=None):
    args = _parser().parse_args(argv)
    if args.command == "bbme":
        import bbme
        return bbme.main(args)
    if args.command == "results":
        import motion
        import results
        old = motion.BBME_BLOCK_SIZE, motion.MOTION_VECTOR_ERROR_THRESHOLD_PERCENTAGE
        try:
            if args.suggest:
                import os
                import roadmap
                import utils
                frames = utils.get_video_frames(os.path.join("resources", "videos", args.path))
                fd = int(args.fd) if args.fd is not None else results.FRAME_DISTANCE
                mid = max(fd, len(frames) // 2)
                hint = roadmap.suggest_parameters(frames[mid - fd], frames[mid])
                print("suggested for this video: {}".format(hint))
                motion.BBME_BLOCK_SIZE = hint["block_size"]
                motion.MOTION_VECTOR_ERROR_THRESHOLD_PERCENTAGE = hint["outlier_fraction"]
            if args.block_size is not None:
                motion.BBME_BLOCK_SIZE = args.block_size
            if args.outlier_fraction is not None:
                motion.MOTION_VECTOR_ERROR_THRESHOLD_PERCENTAGE = args.outlier_fraction
            return results.main(args)
        finally:
            motion.BBME_BLOCK_SIZE, motion.MOTION_VECTOR_ERROR_THRESHOLD_PERCENTAGE = old
    if args.command == "suggest":
        import roadmap
        import utils
        frames = utils.get_video_frames(args.path)
        out = roadmap.suggest_parameters(frames[args.fi - args.fd], frames[args.fi])
        print("frame shape: {}".format(frames[0].shape))
        for k, v in out.items():
            print("{}: {}".format(k, v))
        return out
    if args.command == "projective":
        return _projective(args)
    if args.command == "stabilize":
        return _stabilize(args)
    if args.command == "mosaic":
        return _mosaic(args)
    if args.command == "subpel":
        return _subpel(args)
    if args.command == "hier":
        return _hier(args)
    if args.command == "vbs":
        return _vbs(args)
    if args.command == "bipred":
        return _bipred(args)
    if args.command == "gmc":
        return _gmc(args)
    if args.command == "prop":
        return _prop(args)
    if args.command == "interp":
        return _interp(args)
    if args.command == "retime":
        return _retime(args)
    if args.command == "obmc":
        return _obmc(args)
    if args.command == "denoise":
        return _denoise(args)
    import _gme_native
    import roadmap
    print("searching procedures (-sp): 0 exhaustive, 1 three-step, 2 2-D log, 3 diamond   (bbme.py:609-614)")
    print("norms: 0 MAE, 1 MSE (bbme.py:608; the bbme script always uses MSE, as upstream)")
    print("motion models (roadmap.global_motion_estimation): " + ", ".join(roadmap.MODELS))
    print("sub-pel refinement (gme_cli.py subpel --levels): 0 integer, 1 half-pel, 2 quarter-pel   (subpel.py)")
    print("hierarchical search (gme_cli.py hier): --levels 1 .. 3, -cw 0 .. 8, -r 0 .. 3, block size a multiple of 2^(levels-1) up to 64   (hier.py)")
    print("variable block size (gme_cli.py vbs): --depth 0 .. 2, -r 0 .. 3, --penalty 0 .. 2^30, roots a multiple of 2^depth up to 64, leaves of at least 4   (vbs.py)")
    print("bidirectional prediction (gme_cli.py bipred): -bs 4 .. 64, -r 0 .. 2, --rounds 0 .. 2, --penalty 0 .. 2^30; per block the past frame, the next one or their average   (bipred.py)")
    print("global motion compensation (gme_cli.py gmc): -bs 4 .. 64, --penalty 0 .. 2^30, --estimator projective | affine; per block the camera warp or the block's own vector   (gmc.py)")
    print("vector propagation search (gme_cli.py prop): -bs 4 .. 64, --rounds 1 .. 4, --steps 0 .. 4, --camera projective | affine | none; own, neighbour, temporal, camera and zero vectors on a prior field, refined by one pixel   (propagate.py)")
    print("frame interpolation (gme_cli.py interp): -bs 4 .. 64, -sw 0 .. 8, --bias 0 .. 2^16, --upconvert; the frame halfway between two frames by a bilateral search, borders replicated   (interp.py)")
    print("frame retiming (gme_cli.py retime): -bs 4 .. 64, -sw 0 .. 16, --bias 0 .. 2^16, --rate-in A --rate-out B | --slow K | -fi I --phase n/d (d <= 64); the frame at any phase between two frames by a bilateral quarter-pel search, frame-rate conversion and slow motion   (retime.py)")
    print("overlapped block compensation (gme_cli.py obmc): -bs 4 .. 64, --subpel 0 .. 2, --hier; every pixel blended from its block's and the nearest neighbours' predictions under a linear ramp, borders replicated   (obmc.py)")
    print("temporal denoising (gme_cli.py denoise): -bs 4 .. 64, --radius 1 .. 2, --subpel 0 .. 2, --strength 1 .. 64 (default 24, a convention); every frame averaged with the overlapped predictions of it from its neighbours, each pixel gated by its 3 x 3 prediction error   (denoise.py)")
    try:
        print("device: " + _gme_native.default_context().info()["name"])
    except Exception as e:      # noqa: BLE001 -- no GPU: say so, the listing above is still useful
        print("device: none (%s)" % e)
    return None


if __name__ == "__main__":
    main(sys.argv[1:])
