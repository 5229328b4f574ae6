"""Command-line options (reference: model_option.py:5-89): same flag names and defaults; list-typed flags
are parsed properly, and the multi-GPU / precision flags the reference lacks are added."""
import argparse


def _ids(text):
    return [t if t == "s" else int(t) for t in str(text).replace(",", " ").split()]


def options(argv=None):
    p = argparse.ArgumentParser(description="MI355X self-supervised depth training")
    p.add_argument("--datapath", type=str, default="./dataset/kitti")
    p.add_argument("--splits", type=str, default="./splits")
    p.add_argument("--dataset", type=str, default="synthetic", choices=["kitti_mono", "kitti_stereo", "synthetic"])
    p.add_argument("--datatype", type=str, default="kitti_eigen_zhou")
    p.add_argument("--epoch", type=int, default=24)
    p.add_argument("--batch", type=int, default=12)
    p.add_argument("--prepetch", type=int, default=2)
    p.add_argument("--num_workers", type=int, default=None,
                   help="DataLoader workers per process.  Default: 12 (the reference's, model_option.py:32-34) for fp32 networks, 24 "
                        "with --amp bf16, whose step consumes ~1500 samples/s (12 workers deliver ~700-860 with --gpu_image_prep, 16 "
                        "~1100, 24 ~1200 on a 16-core share: tools/loader_cost.py --workers N); -1 = sized from this rank's share of "
                        "the host cores")
    p.add_argument("--learning_rate", type=float, default=1e-4)
    p.add_argument("--scheduler_step", type=int, default=15)
    p.add_argument("--disp_smoothness", type=float, default=1e-3)
    p.add_argument("--save", type=str, default="mono")
    p.add_argument("--height", type=int, default=192)
    p.add_argument("--width", type=int, default=640)
    p.add_argument("--scales", type=_ids, default=[0, 1, 2, 3])
    p.add_argument("--min_depth", type=float, default=0.1)
    p.add_argument("--max_depth", type=float, default=100.0)
    p.add_argument("--frame_ids", type=_ids, default=[0, -1, 1])
    p.add_argument("--pose_frames", type=str, default="pair", choices=["pair", "all"])
    p.add_argument("--num_layers", type=int, default=18, choices=[18, 34, 50, 101, 152])
    p.add_argument("--weight_init", type=lambda s: str(s).lower() in ("1", "true", "yes"), default=True)
    p.add_argument("--pose_type", type=str, default="separate", choices=["posecnn", "shared", "separate"])
    p.add_argument("--use_automasking", type=lambda s: str(s).lower() in ("1", "true", "yes"), default=True)
    # additions
    p.add_argument("--fused", type=lambda s: str(s).lower() in ("1", "true", "yes"), default=True)
    p.add_argument("--fused_train", type=lambda s: str(s).lower() in ("1", "true", "yes"), default=True,
                   help="one launch for every scale's photometric term and its gradient (csrc/photo_train.hip)")
    p.add_argument("--uint8_loader", type=lambda s: str(s).lower() in ("1", "true", "yes"), default=True,
                   help="colours stay uint8 through the DataLoader; x/255 happens on the GPU (same values, 1/4 of the bytes)")
    p.add_argument("--collate_step_keys", type=lambda s: str(s).lower() in ("1", "true", "yes"), default=True,
                   help="DataLoader workers stack only the entries a step reads")
    p.add_argument("--graph", type=lambda s: str(s).lower() in ("1", "true", "yes"), default=True,
                   help="single-GPU training: capture the step into one hipGraph and replay it (host launch cost off the critical path)")
    p.add_argument("--graph_valid", type=lambda s: str(s).lower() in ("1", "true", "yes"), default=True,
                   help="with --graph: capture the validation step (no grad, networks in eval mode) into a hipGraph of its own too")
    p.add_argument("--device_prefetch", type=lambda s: str(s).lower() in ("1", "true", "yes"), default=True,
                   help="upload the next batch on a side stream while the current step computes")
    p.add_argument("--gpu_image_prep", type=str, default="auto", choices=["auto", "true", "false"],
                   help="KITTI loaders: workers only decode; flip, Lanczos pyramid, colour jitter and ToTensor run on the GPU "
                        "(bit-equal to Pillow; csrc/imgproc.hip).  auto = on when training on a GPU")
    p.add_argument("--gpu_velodyne", type=int, default=0, choices=[0, 1],
                   help="KITTI loaders, honoured only with gpu_image_prep on: the workers hand the velodyne scans over and the ground-truth "
                        "map is projected on the GPU (bit-equal to point2depth; csrc/velodyne.hip).  Off by default.  Measured "
                        "(tools/velodyne_cost.py, profiles/r13_velodyne_*, LABNOTES 'Velodyne ground truth'): ~75 us per batch of 12 on "
                        "the GPU against ~27 us for the scatter it replaces; one worker's time per sample 7.2 -> 5.7 ms; no measurable "
                        "gain in loader samples/s with 24 workers")
    p.add_argument("--synthetic_raw", action="store_true",
                   help="synthetic dataset hands over KITTI-sized decoded frames (1242x375 uint8), as the KITTI loaders do with gpu_image_prep")
    p.add_argument("--resume", type=int, default=0,
                   help="restart after this many finished epochs from ./model_save/<save>/ (weights <key><N>.pt + state<N>.pt)")
    p.add_argument("--native_adam", type=int, default=1,
                   help="GPU: torch.optim.Adam(fused=True) with its step as ONE launch (mdx/optim.py, csrc/adam.hip); 0: torch's own step")
    p.add_argument("--clip_grad_norm", type=float, default=0.0,
                   help="clip the gradients to this global L2 norm inside the optimiser step, decided on the device (mdx/optim.py: "
                        "max_grad_norm; three launches, capturable); 0: off")
    p.add_argument("--skip_nonfinite", type=int, default=0,
                   help="1: a step whose global gradient norm is not finite changes no weight, moment or step count (decided on the "
                        "device; counted, printed after each epoch)")
    p.add_argument("--ema_decay", type=float, default=0.0,
                   help="keep an exponential moving average of the weights and batch-norm statistics with this decay, e.g. 0.999, updated "
                        "on the device after every optimiser step (mdx/optim.py: WeightEMA, csrc/ema.hip; capturable); 0: off.  Trainer only: model_test.py always evaluates the live encoder<N>.pt / "
                        "decoder<N>.pt; model_ema_eval.py evaluates the averaged ema_<key><N>.pt with this option set")
    p.add_argument("--ema_warmup", type=int, default=1,
                   help="with --ema_decay: update t uses min(decay, (1 + t) / (10 + t)), so the early average follows the weights")
    p.add_argument("--ema_valid", type=int, default=1,
                   help="with --ema_decay: each epoch's validation runs on the averaged weights (exchanged in place and put back)")
    p.add_argument("--check_weights", type=int, default=0,
                   help="N > 0: before the first step, after every N-th step and before each checkpoint, digest the float32 master "
                        "weights on the device (mdx/optim.py: WeightDigest, csrc/digest.hip) and, in a data-parallel run, compare the "
                        "digests across the ranks (one int64 all-reduce; a difference raises on every rank); state<N>.pt records the "
                        "digests and --resume verifies the weight files against them; 0: off")
    p.add_argument("--grad_stats", type=int, default=0,
                   help="N > 0: after every N-th step, one read-only pass on the device over every trained parameter and its gradient "
                        "(mdx/optim.py: GradStats, csrc/tensor_stats.hip): per-tensor norms, largest magnitudes, counts of non-finite "
                        "and zero elements, and a per-tensor history kept on the device and read once per epoch -- rank 0 prints the "
                        "tensors with the largest and smallest gradient norm, names the tensors whose gradients or weights went "
                        "non-finite with the step it first happened, and appends a line to ./model_save/<save>/grad_stats.jsonl.  "
                        "The gradients are the unclipped ones; the history is not saved and does not survive --resume; 0: off")
    p.add_argument("--loss_stats", type=int, default=0,
                   help="N > 0: after every N-th step, one read-only pass on the device over the maps the loss path leaves behind "
                        "(mdx/loss_stats.py: LossStats, csrc/loss_stats.hip): per scale and image the share of the pixels the auto-mask "
                        "removed, the share each source frame won, the range of the disparity, counts of corrupt indices and non-finite "
                        "disparities, and a per-scale history kept on the device and read once per epoch -- rank 0 prints one line per "
                        "scale and appends a line to ./model_save/<save>/loss_stats.jsonl.  The history is not saved and does not "
                        "survive --resume; 0: off")
    p.add_argument("--loss_stats_static", type=float, default=0.9,
                   help="--loss_stats: an image counts as static when at least this share of its pixels is auto-masked (a reporting "
                        "threshold, in (0, 1])")
    p.add_argument("--depth_supervision", type=float, default=0.0,
                   help="W > 0: semi-supervised training from the sparse lidar ground truth of the batch, (\"depth\", 0): W * the mean "
                        "over the scales of a Charbonnier penalty (eps 1e-3) on log depth - log ground truth, the depth that of the "
                        "scale's disparity resampled to the ground truth's size, over the pixels with --min_depth < gt < --max_depth, "
                        "divided by their number (csrc/sparse_depth.hip, model_loss.SparseDepthLoss; forward and gradient on the "
                        "device, capturable, bit-reproducible).  It gives a mono-only run a metric scale.  A data-parallel run "
                        "normalises by each rank's OWN valid count, so the exchanged gradient is the mean of the ranks' terms, not the "
                        "term of the pooled batch.  Prints one line per epoch.  0: off, no loss module is made and none of its kernels run.  Measured "
                        "(tools/sparse_depth_cost.py, profiles/r14_sparse_depth_cost.txt, LABNOTES 'Sparse lidar supervision'): "
                        "batch 12 at 192x640 under 375x1242 ground truth, 4.5 %% valid: forward + backward 265 us in 6 launches against 2016 us "
                        "in 200 launches for the same term in torch ops; the training loop's step -- the captured step and the five eager launches behind "
                        "it that keep the epoch's sums -- 14.66 -> 15.01 ms (+2.4 %%)")
    p.add_argument("--stereo_hints", type=float, default=0.0,
                   help="W > 0: proxy depth from the rectified stereo pair of the batch -- needs \"s\" in --frame_ids and inputs[\"stereo\"]: "
                        "a census + semi-global matcher (9x7 census, eight paths, P1 8, P2 64, left-right check, sub-pixel parabola; "
                        "csrc/stereo_hints.hip, include/mdx.h has the definition) over the un-augmented (\"color\", 0, 0) and "
                        "(\"color\", \"s\", 0) gives depth = fx * baseline / disparity where the check holds, and W * the mean over the "
                        "scales of the --depth_supervision penalty against it joins the loss (a second model_loss.SparseDepthLoss; "
                        "may be on together with --depth_supervision).  On the device, inside the captured step, bit-reproducible.  A "
                        "data-parallel run normalises by each rank's OWN valid count, so the exchanged gradient is the mean of the "
                        "ranks' terms, not the term of the pooled batch.  Prints one line per epoch.  0: off, no module, no workspace, "
                        "none of its kernels run.  No KITTI accuracy has been measured with it: the claim is that the hints are what "
                        "the definition says.  Measured (tools/stereo_hints_cost.py, profiles/r16_stereo_hints_cost.txt, LABNOTES "
                        "'Stereo proxy depth'): batch 12 at 192x640: the matcher 1.74 ms per call at 64 disparities (12 launches; its path passes move 2.83 GB, 0.35 ms at 8 TB/s: latency-bound walks), 3.71 ms at 128; the training loop's step at frame_ids 0 -1 1 s -- the captured step and the eager launches behind it that keep the epoch's sums -- 14.68 -> 16.85 ms (+14.8 %%)")
    p.add_argument("--stereo_hints_disp", type=int, default=64, choices=[64, 128],
                   help="--stereo_hints: the disparities searched.  At 640 columns fx * 0.1 = 37.1, so 64 reaches down to a depth of 0.58 "
                        "units (about 3.1 m); nearer pixels fail the left-right check and get no hint")
    p.add_argument("--stereo_hints_select", action="store_true",
                   help="--stereo_hints W > 0 only (it means nothing without it): a hint supervises a pixel only where warping the stereo "
                        "partner with the hint depth gives a strictly lower SSIM + L1 reprojection loss against the target than warping it "
                        "with the depth of the step's own finest disparity (the rule of Watson et al. 2019 through the stereo view alone, "
                        "not the minimum over all sources; include/mdx.h 'depth-hint selection', csrc/hint_select.hip, DESIGN.md 4.7); "
                        "the selected map goes to the same term, the epoch line carries the kept share.  Default off: no call, no "
                        "workspace.  No KITTI accuracy has been measured with it.  Measured (tools/hint_select_cost.py, profiles/r17_hint_select_cost.txt, LABNOTES "
                        "'Depth-hint selection'): batch 12 at 192x640: 0.047 ms per call in 2 launches against 0.199 ms in about 17 for the same result from "
                        "the fine-grained ops; the training loop's step at frame_ids 0 -1 1 s with --stereo_hints 0.05 16.90 -> 16.97 ms (+0.44 %%)")
    p.add_argument("--shadow_weights", type=int, default=1,
                   help="--amp bf16: cast every convolution weight once per step by one launch (mdx/shadow.py); 0: autocast's cast per convolution")
    p.add_argument("--fused_tail", type=int, default=1,
                   help="GPU: the loss as one autograd node, the pose head's output -> projections in one launch (0: the reference's small torch ops)")
    p.add_argument("--overlap_pose", type=int, default=1,
                   help="1: the separate pose network runs on a side stream beside the depth network, forward and backward (many of "
                        "their kernels are too small to fill the GPU alone: +13 %% fp32, +32 %% bf16 on one MI355X); 0: one after the other")
    p.add_argument("--synthetic_geometry", action="store_true",
                   help="synthetic dataset: frames rendered from one rigid textured scene at known poses, ground truth = its "
                        "depth (model_tool/synthetic.py: scene) -- for tests of what the step learns")
    p.add_argument("--synthetic_pool", type=int, default=0, help="synthetic dataset: number of distinct samples kept (0 = all)")
    p.add_argument("--noise", type=str, default="device", choices=["device", "cpu"])
    p.add_argument("--grad_comm", type=str, default="fp32", choices=["fp32", "bf16"],
                   help="data parallel: dtype of the gradient all-reduce (bf16 halves the bytes over xGMI; gradients rounded once)")
    p.add_argument("--bucket_mb", type=int, default=0,
                   help="data parallel: size of an all-reduce bucket (0 = one bucket for a captured step, 32 MB eager)")
    p.add_argument("--amp", type=str, default="none", choices=["none", "bf16"])
    p.add_argument("--channels_last", type=str, nargs="?", const="all", default="auto",
                   help='stages whose maps are channels-last (NHWC): "none", "all", "auto" (= mdx.layout.DEFAULT_PLAN, the '
                        'measured fastest) or a list of stem,layer1..layer4,decoder,pose (mdx/layout.py)')
    p.add_argument("--synthetic_length", type=int, default=768)
    p.add_argument("--max_steps", type=int, default=0, help="stop an epoch early (0 = full epoch)")
    p.add_argument("--miopen_find", action="store_true",
                   help="cudnn.benchmark: MIOpen find mode (a search of minutes for shapes that are not in the "
                        "shipped find-db; the default, immediate mode, already uses the db)")
    o = p.parse_args(argv)
    if o.num_workers is None:
        o.num_workers = 24 if o.amp == "bf16" else 12
    return o
