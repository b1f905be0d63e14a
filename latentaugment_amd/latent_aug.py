"""Host-side mirror of augments/utils/util_latent_aug.py::LatentAug for the MI355X path.

Same constructor fields (read from `opt`), same `forward(w, fname) -> (img, w_aug)` contract, same attributes
(`num_ws, w_dim, z_dim, stats_dataset_w`).  The N-step optimisation itself is one call into the C ABI
(`la_latent_opt_run`); this file only moves tensors to the device, draws the crop position on the host and -- when a
process group is active -- shards independent samples over ranks and gathers the result with ONE collective.
`opt` is parsed once into a `loop_options.LoopOptions` record and never written; the handle that runs the loop, its engines and
the device-resident banks are `loop_handle.LoopHandle` / `LoopBanks` (a stream lane is one more such handle over the same banks).

Differences from the reference, all deliberate:
  * one process per GPU + torch.distributed (RCCL) instead of single-process nn.DataParallel (:28-33);
  * works with `gpu_ids=[k]` only on a ROCm device: there is no CPU path here (the reference's CPU path is the oracle);
  * G / banks can be injected (no pickle / zip needed for synthetic runs); on-disk formats are the next scope row;
  * the final synthesis uses explicit noise tensors drawn on the host RNG when noise_strength != 0 (defect g).
"""
import ctypes as C
import os
import random

import numpy as np
import torch

from . import _lib
from .loop_handle import LoopBanks, LoopHandle, load_perceptual_net
from .loop_options import (LoopOptions, center_crop_geometry, get_params, lanes_eligible,      # noqa: F401  (re-exported)
                           resolve_perceptual_net)
from .synthesis import MappingEngine


def write_png_gray(path, a):
    """8-bit greyscale PNG of a 2-D uint8 array (the reference writes its snapshots with cv2.imwrite, :655)."""
    import struct
    import zlib
    a = np.ascontiguousarray(a, dtype=np.uint8)
    h, w = a.shape
    raw = b''.join(b'\x00' + a[y].tobytes() for y in range(h))

    def chunk(tag, data):
        return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xffffffff)
    with open(path, 'wb') as f:
        f.write(b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 0, 0, 0, 0)) + chunk(b'IDAT', zlib.compress(raw, 6)) +
                chunk(b'IEND', b''))


def write_curve_png(path, values, width=480, height=320, margin=24):
    """Line plot of a sequence as an 8-bit greyscale PNG: frame, polyline, nothing else (the reference draws its per-key curves
    with matplotlib, snapshot_stats :620-633; matplotlib is not a dependency here, so there are no tick labels or legend --
    the numbers are in the .jsonl next to the picture)."""
    v = np.asarray(list(values), dtype=np.float64)
    img = np.full([height, width], 255, dtype=np.uint8)
    x0, x1, y0, y1 = margin, width - margin - 1, margin, height - margin - 1
    img[y0, x0:x1 + 1] = img[y1, x0:x1 + 1] = 0
    img[y0:y1 + 1, x0] = img[y0:y1 + 1, x1] = 0
    if v.size and np.isfinite(v).any():      # (an all-NaN / all-inf curve: frame only)
        v = np.where(np.isfinite(v), v, np.nan)
        lo, hi = float(np.nanmin(v)), float(np.nanmax(v))
        span = hi - lo if hi > lo else 1.0
        xs = np.full(v.size, (x0 + x1) // 2) if v.size == 1 else np.round(x0 + 4 + (x1 - x0 - 8) * np.arange(v.size) / (v.size - 1)).astype(int)
        ys = np.round(y1 - 4 - (y1 - y0 - 8) * (np.nan_to_num(v, nan=lo) - lo) / span).astype(int)
        for i in range(v.size):
            img[max(ys[i] - 2, 0):ys[i] + 3, max(xs[i] - 2, 0):xs[i] + 3] = 0          # marker
            if i + 1 < v.size:
                n = int(max(abs(xs[i + 1] - xs[i]), abs(ys[i + 1] - ys[i]), 1))
                for t in range(n + 1):                                                 # segment, one pixel per step along the longer axis
                    img[int(round(ys[i] + (ys[i + 1] - ys[i]) * t / n)), int(round(xs[i] + (xs[i + 1] - xs[i]) * t / n))] = 64
    write_png_gray(path, img)


def shard_bounds(batch, world_size, rank):
    """Contiguous sample range of a rank: [rank*b, (rank+1)*b) with b = ceil(batch / world_size)."""
    per = (batch + world_size - 1) // world_size
    lo = min(rank * per, batch)
    hi = min(lo + per, batch)
    return lo, hi, per


def sharded(group=None):
    """True where forward() shards the batch over a process group: an initialised group of more than one rank.  (A group of ONE rank
    takes the same path -- broadcast, shard, all_gather -- when LATENTAUG_FORCE_SHARDED=1: the RCCL rehearsal of a 1-GPU box.)"""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return False
    return dist.get_world_size(group) > 1 or os.environ.get('LATENTAUG_FORCE_SHARDED') == '1'


def gather_shards(local, per, batch, group=None):
    """ONE all_gather of equally padded shards -> the full batch on every rank (the reference gathers to gpu_ids[0])."""
    import torch.distributed as dist
    world = dist.get_world_size(group)
    dev = local.device
    # RCCL ('nccl') gathers device buffers directly over xGMI; a gloo group (CPU rehearsal / tests) is staged through host
    stage = dev.type == 'cuda' and dist.get_backend(group) == 'gloo'
    pad = torch.zeros([per] + list(local.shape[1:]), dtype=local.dtype, device='cpu' if stage else dev)
    pad[:local.shape[0]] = local
    out = torch.empty([world * per] + list(local.shape[1:]), dtype=local.dtype, device=pad.device)
    dist.all_gather_into_tensor(out, pad, group=group)
    return out[:batch].to(dev)


def broadcast_controls(crop_pos, group=None, device=None, host_group=None):
    """Rank 0's per-forward host draws -- (crop x, crop y, 48-bit seed of the final-synthesis noise) -- to every rank of the
    group.  Control plane only (three integers through the host); the data path keeps its single all_gather.  `host_group`: a gloo
    group over the same ranks.  Through an RCCL group the object broadcast reads its size back on the host, which waits for the
    RCCL stream, which waits for everything this rank has queued: the previous batch drains before the next one is enqueued.  Over
    the host group the ranks still meet here, but no GPU queue is involved and batches stay queued back to back."""
    import torch.distributed as dist
    ctl = [None]
    if dist.get_rank(group) == 0:
        ctl[0] = (int(crop_pos[0]), int(crop_pos[1]), random.getrandbits(48))
    src = dist.get_global_rank(group, 0) if group is not None else 0
    if host_group is not None:
        dist.broadcast_object_list(ctl, src=src, group=host_group, device=torch.device('cpu'))
        return ctl[0]
    on_host = dist.get_backend(group) == 'gloo' or device is None
    dist.broadcast_object_list(ctl, src=src, group=group, device=torch.device('cpu') if on_host else device)
    return ctl[0]


def host_control_group(group=None, device=None):
    """A gloo group over the ranks of the default (RCCL) group, for broadcast_controls; None where the data group is gloo already, is
    a sub-group (dist.new_group must be entered by EVERY process of the job, which only the default group guarantees here), or
    LATENTAUG_CTL_DEVICE=1 asks for the device path.  Collective: every rank of the default group calls it at the same point (the
    first sharded forward)."""
    import torch.distributed as dist
    if group is not None or dist.get_backend() == 'gloo' or os.environ.get('LATENTAUG_CTL_DEVICE') == '1':
        return None
    if not dist.is_gloo_available():
        return None
    try:
        g = dist.new_group(backend='gloo')
    except Exception as e:       # (e.g. no usable network interface for gloo on this host)
        print(f'[latentaugment_amd] no gloo control group ({type(e).__name__}: {e}); control broadcast stays on the device path')
        g = None
    # every rank must take the same path: agree over the data group that all of them got their host group
    ok = torch.tensor([1 if g is not None else 0], device=device if device is not None else torch.device('cuda', torch.cuda.current_device()), dtype=torch.int32)
    dist.all_reduce(ok, op=dist.ReduceOp.MIN)
    return g if int(ok.item()) == 1 else None


class InMemoryLatentCodes:
    """Minimal stand-in for util_dataset.LatentCodeDataset: fname -> inverted latent [num_ws, w_dim] (or [w_dim])."""

    def __init__(self, codes):
        self.codes = dict(codes)

    def lookup(self, fname):
        return np.asarray(self.codes[fname], dtype=np.float32)


class LatentAug:
    def __init__(self, phase, opt, save_dir, gpu_ids, generator=None, discriminator=None, banks=None, latent_codes=None,
                 feature_net=None, group=None):
        self.save_dir = save_dir
        self.phase = phase
        self.group = group
        self._ctl_group = None      # gloo companion of an RCCL group for the per-forward control broadcast (host_control_group)
        if not gpu_ids:
            raise _lib.LatentAugHipError(
                'LatentAug (MI355X path) needs a GPU id in gpu_ids_aug; the CPU restatement lives in oracle/ and is '
                'test infrastructure only')
        if len(gpu_ids) > 1:
            raise _lib.LatentAugHipError(
                'one process drives one GPU: launch one rank per GPU (torch.distributed / RCCL) instead of passing '
                'several gpu_ids to a single process')
        self.device = torch.device('cuda', gpu_ids[0])
        o = self.options = LoopOptions.from_opt(opt)      # `opt` is read here, once, and never written
        self.res, self.batch_size, self.modalities = o.img_resolution, o.batch_size, list(o.modalities)
        self.num_epochs, self.opt_lr, self.truncation_psi = o.opt_num_epochs, o.opt_lr, o.truncation_psi
        self.w_pix, self.w_lpips, self.w_latent, self.w_disc = o.w_pix, o.w_lpips, o.w_latent, o.w_disc
        self.crop_size, self.preprocess = o.crop_size_aug, o.preprocess_aug
        self.soft_aug, self.alpha, self.verbose_log = o.soft_aug, o.alpha, o.verbose_log
        self.criterion_mode, self.final_noise_mode, self.precision = o.criterion_mode, o.final_noise_mode, o.precision
        self.latent_space, self.wplus = o.latent_space, o.wplus
        self.hip_graph, self.overlap_criteria = o.hip_graph, o.overlap_criteria
        self.stream_lanes = o.stream_lanes      # (assignable: bench.py switches the lanes off and on again around its single-loop leg)
        resolved = resolve_perceptual_net(o, feature_net)      # (a missing weight file is reported before anything touches a device)
        if generator is None:
            generator, discriminator = self._load_networks(discriminator)
        self._generator = generator
        self._mapping = None
        self._max_local = self._local_capacity()
        pnet = load_perceptual_net(resolved, self.device, o.crop_size_aug)
        self.banks = LoopBanks(o, phase, self.device, banks, latent_codes)
        self._loop = LoopHandle(o, generator, discriminator, pnet, self.banks, self._max_local, self.device)
        self._lib = self._loop._lib
        self.engine, self.disc, self.feat = self._loop.engine, self._loop.disc, self._loop.feat
        self.W, self.Xc, self.Fbank = self.banks.W, self.banks.Xc, self.banks.Fbank
        self.center_crop, self.center_off = self.banks.center_crop, self.banks.center_off
        self.loop_window = self._loop.loop_window
        self.num_ws, self.w_dim = self.engine.num_ws, self.engine.w_dim
        self.z_dim = getattr(generator, 'z_dim', self.w_dim)
        self.stats_dataset_w = self.banks.latent_codes
        self.stats_loss = {}
        self.stats_time = {}
        self._verbose_flag = o.verbose_log      # the reference logs the FIRST batch only (:189-191, :297-300)
        # stream lanes: a full local batch as two interleaved half-batch loops on two HIP streams, each a LoopHandle of its own
        # (loop / synthesis / discriminator / feature handles) over the same banks and the same resolved perceptual net.
        self._lane_parts = (generator, discriminator, pnet)
        self._lanes = None
        self._lane_stream = None
        self.lanes_active = False           # the last batch went through the lanes
        self.lanes_concurrent = True        # False: the lanes one after the other on one stream (bench.py's per-launch brackets)
        # First-batch self-check of the concurrent lanes (`opt.lanes_selfcheck`, default on): the first full batch runs through the lanes
        # one after the other AND side by side; the two must agree bit for bit (they are the same launches), otherwise this handle
        # warns and keeps the lanes serial.  Why: rounds 2-3 saw wrong results whenever two queues of this library overlapped; round 4
        # traced it to packed-FP32 instructions and removed them (DESIGN 8 'Two streams'), but the hardware mechanism is not pinned
        # down, so the product checks the property it relies on where it relies on it instead of trusting one toolchain's codegen.
        self.lanes_selfcheck = None         # None: not run yet | 'bit-identical' | 'differs: lanes serial from now on' | 'off'
        # the lanes' handles and workspaces exist from construction on (an allocation failure surfaces here, not inside the first batch)
        if self.lanes_eligible(self._max_local):
            self.build_lanes()

    def _load_networks(self, discriminator):
        """load_stylegan (reference :466-484): <model_dir>/<dataset>/training-runs/<dataset_name>/<modalities>/<exp>/<pkl>"""
        from . import formats
        o = self.options
        path = formats.find_network_pkl(o.model_dir, o.dataset_aug, o.dataset_name_aug, self.modalities, o.exp_stylegan,
                                        o.network_pkl_stylegan)
        print(f'Loading stylegan from "{path}"...')
        nets_ = formats.load_network_pkl(path)
        return nets_['G_ema'], discriminator if discriminator is not None else nets_.get('D')

    def _local_capacity(self):
        """Per-process capacity: the whole batch, or -- with an active process group, where forward() hands this rank only its shard --
        ceil(batch / world) (`opt.max_local_batch` overrides)."""
        max_local = self.batch_size
        try:
            import torch.distributed as dist
            if sharded(self.group):
                max_local = (self.batch_size + dist.get_world_size(self.group) - 1) // dist.get_world_size(self.group)
        except (RuntimeError, ValueError):
            pass
        return int(self.options.max_local_batch or max_local)

    @property
    def _h(self):
        return self._loop._h

    # ------------------------------------------------------------------ helpers (reference :493-498)
    def broadcasting(self, latent):
        return latent.repeat([1, self.num_ws, 1])

    @staticmethod
    def reverse_broadcasting(latent):
        return latent[:, :1, :]

    # ------------------------------------------------------------------ the hot path
    def crop_window(self, crop_pos):
        """Absolute (x, y) of the crop_size_aug window for a position drawn by get_params (LoopOptions.crop_window)."""
        return self.options.crop_window(crop_pos)

    @property
    def latent_rows(self):
        """Rows of one sample's optimised latent: 1 in W space, num_ws in W+."""
        return self.num_ws if self.wplus else 1

    def _crop_pos(self, crop_pos=None):
        """The given crop position, else the one forward() drew for this batch, else a fresh draw."""
        cp = getattr(self, 'crop_params', None)
        return crop_pos if crop_pos is not None else cp['crop_pos'] if cp else get_params(self.res, self.crop_size, self.preprocess)['crop_pos']

    def _empty_pair(self, b):
        """Uninitialised (img [b,C,R,R], w_aug [b,num_ws,w_dim]) on the current stream."""
        return self._loop.empty_pair(b)

    def _shard_noises(self, noises, B, lo, hi, seed):
        """Final-synthesis noise of samples lo:hi of a batch of B: the caller's rows, else rows of the batch's seeded draw, else None."""
        if noises is not None:
            return [t[lo:hi].contiguous() if t is not None else None for t in noises]
        return self.engine.make_noises(B, batch_seed=seed, rows=(lo, hi)) if self.options.final_noise_code == 2 else None

    def _gather_pair(self, img, w_aug, per, B, ev=None):
        """This rank's rows -> the full batch: image and latent packed into a single buffer, ONE collective per batch (ev: its shard_timers events).
        The widths are explicit: a rank with an empty shard packs 0 rows, and reshape(0, -1) is refused."""
        n_img = self.engine.img_channels * self.res * self.res
        flat = torch.cat([img.reshape(img.shape[0], n_img), w_aug.reshape(w_aug.shape[0], self.num_ws * self.w_dim)], dim=1)
        if ev is not None:
            ev[1].record()
        full = gather_shards(flat, per, B, self.group)
        if ev is not None:
            ev[2].record()
        return full[:, :n_img].reshape(B, self.engine.img_channels, self.res, self.res), full[:, n_img:].reshape(B, self.num_ws, self.w_dim)

    def run_local(self, w, final_noises=None, want_losses=False, crop_pos=None, trace=None, out=None):
        """w [b,1,w_dim] on this device (W+: [b,num_ws,w_dim]) -> (img [b,C,R,R], w_aug [b,num_ws,w_dim], losses or None).
        out (optional): (img, w_aug) tensors to fill instead of allocating them on the current stream.
        trace (optional): dict that receives the per-step snapshots 'w' [steps,b,w_dim] (latent after the step; W+:
        [steps,b,num_ws,w_dim]) and 'img' [steps,b,C,R,R]; trace['want'] (default ('w', 'img')) selects them, and may name 'grad'
        (dL/dw, the shape of 'w')."""
        xy = self.crop_window(self._crop_pos(crop_pos)) if self.feat is not None else None
        return self._loop.run(w, final_noises, want_losses, xy, trace, out)      # (the handle keeps final_noises alive: LoopHandle.run)

    # ---- stream lanes: the local batch as two interleaved half-batch loops on two HIP streams
    def lanes_eligible(self, b):
        """Whether a local batch of b goes through the two lanes (loop_options.lanes_eligible, on this object's own fields:
        `stream_lanes` may have been reassigned since construction)."""
        return lanes_eligible(self, self._max_local, b)

    def build_lanes(self):
        generator, discriminator, pnet = self._lane_parts
        lane = self.options.lane(self._max_local)
        self._lanes = [LoopHandle(lane, generator, discriminator, pnet, self.banks, lane.max_local_batch, self.device) for _ in range(2)]
        self._lane_stream = torch.cuda.Stream(device=self.device)

    def run_lanes(self, w, final_noises=None, crop_pos=None, concurrent=True):
        """run_local for a full local batch through the two lanes: samples 0, 2, 4, .. on the current stream, samples 1, 3, 5, .. on the
        lane stream (forked from / joined into the current stream); every buffer either lane touches is allocated on the current
        stream before the fork.  `concurrent=False` runs the lanes one after the other on the current stream (same launches)."""
        if self._lanes is None:
            self.build_lanes()
        w = w.to(device=self.device, dtype=torch.float32).contiguous()
        b = w.shape[0]
        assert b == self._max_local and b % 2 == 0, 'stream lanes take the full (even) local batch'
        xy = self.crop_window(self._crop_pos(crop_pos)) if self.feat is not None else None
        if self.options.final_noise_code == 2 and final_noises is None:
            final_noises = self.engine.make_noises(b)      # ONE draw for the batch, as the single loop makes it; a lane keeps its rows
        parts, outs, fns = [], [], []
        for k in (0, 1):
            parts.append(w[k::2].contiguous())
            outs.append(self._empty_pair(b // 2))
            fns.append([t[k::2].contiguous() if t is not None else None for t in final_noises] if final_noises is not None else None)
        main = torch.cuda.current_stream(self.device)
        side = self._lane_stream if concurrent else main
        if concurrent:
            side.wait_stream(main)
        self._lanes[0].run(parts[0], fns[0], crop_window_xy=xy, out=outs[0])
        with torch.cuda.stream(side):
            self._lanes[1].run(parts[1], fns[1], crop_window_xy=xy, out=outs[1])
        if concurrent:
            main.wait_stream(side)
        img, w_aug = self._empty_pair(b)
        for k in (0, 1):
            img[k::2] = outs[k][0]
            w_aug[k::2] = outs[k][1]
        # Lifetime hold: the side stream may still be reading these when their last Python reference is gone, and the caching allocator
        # would then hand their memory out again on the main stream.  They live until the next batch through the lanes.
        self._keep_lanes = (parts, outs, fns)
        return img, w_aug, None

    def run_batch(self, w, final_noises=None):
        """The local batch through two stream lanes when it qualifies (lanes_eligible), through the single loop otherwise."""
        self.lanes_active = self.lanes_eligible(w.shape[0])
        if not self.lanes_active:
            return self.run_local(w, final_noises)
        if self.lanes_selfcheck is None and self.lanes_concurrent:
            return self._lanes_first_batch(w, final_noises)
        return self.run_lanes(w, final_noises, concurrent=self.lanes_concurrent)

    def _lanes_first_batch(self, w, final_noises):
        """The first full batch of a handle: lanes one after the other, then side by side, on the same inputs; bit-identical or the
        handle stays serial (see __init__).  Costs one extra batch, once."""
        if not self.options.lanes_selfcheck:
            self.lanes_selfcheck = 'off'
            return self.run_lanes(w, final_noises, concurrent=True)
        if self._lanes is None:
            self.build_lanes()
        if self.options.final_noise_code == 2 and final_noises is None:
            final_noises = self.engine.make_noises(w.shape[0])      # one draw for both runs
        crop_pos = self._crop_pos() if self.feat is not None else None
        ref_img, ref_w, _ = self.run_lanes(w, final_noises, crop_pos=crop_pos, concurrent=False)
        img, w_aug, _ = self.run_lanes(w, final_noises, crop_pos=crop_pos, concurrent=True)
        if torch.equal(img, ref_img) and torch.equal(w_aug, ref_w):
            self.lanes_selfcheck = 'bit-identical'
            return img, w_aug, None
        import warnings
        dw = float((w_aug - ref_w).abs().max())
        self.lanes_selfcheck = 'differs: lanes serial from now on'
        self.lanes_concurrent = False
        warnings.warn(f'latentaugment_amd: the two stream lanes side by side did not reproduce the lanes one after the other on the first '
                      f'batch (max |dw| {dw:.3e}); this handle runs them one after the other from now on (opt.stream_lanes = 1 avoids the '
                      f'lanes altogether)')
        return ref_img, ref_w, None

    # ---- verbose_log artefacts of the first batch (reference :278-300, :620-655)
    def _log_first_batch(self, losses, elapsed, trace, fname, times=None):
        import json
        import pickle
        L = losses.cpu().numpy()
        active = [('loss_latent', 0, self.w_latent), ('loss_disc', 2, self.w_disc), ('loss_pix', 1, self.w_pix), ('loss_lpips', 3, self.w_lpips)]
        for e in range(self.num_epochs):
            st = {name: float(L[e, col]) for name, col, wgt in active if wgt > 0}      # only the active criteria are logged (:233-268)
            st['loss'] = float(-L[e, 0] - L[e, 1] - L[e, 3] + L[e, 2])
            self.stats_loss[f'epoch_{e}'] = st
            # the loop runs on the device without a host round trip per epoch: the times are device times between HIP events around the
            # criteria of the epoch (seconds, the reference's keys; a criterion's bracket holds its loss scalar and its gradient launches --
            # the reference's the forward only, its backward sits in the untimed loss.backward()); without them the batch time spread evenly
            if times is not None:
                self.stats_time[f'epoch_{e}'] = {'time_latent': float(times[e, 0]), 'time_disc': float(times[e, 1]), 'time_pix': float(times[e, 2]),
                                                 'time_lpips': float(times[e, 3]), 'time_epoch': float(times[e, 4])}
            else:
                self.stats_time[f'epoch_{e}'] = {'time_epoch': elapsed / max(self.num_epochs, 1)}
            desc = ''.join(f'{k} {v:<4.2f} ' for k, v in st.items()) + '||| ' + ''.join(f'{k} {v:<4.3f} ' for k, v in self.stats_time[f'epoch_{e}'].items())
            print(f'epoch {e + 1:>4d}/{self.num_epochs}, {desc}')
        if self.save_dir and self.num_epochs > 0:
            os.makedirs(self.save_dir, exist_ok=True)
            for stats, title in ((self.stats_loss, 'losses'), (self.stats_time, 'times [s]')):
                ticks = list(stats.values())
                for key in ticks[0].keys():      # one curve per logged quantity, named as snapshot_stats names them (:620-633)
                    write_curve_png(os.path.join(self.save_dir, f'{title}_{key}.png'), [x[key] for x in ticks])
                with open(os.path.join(self.save_dir, f'{title}.jsonl'), 'w') as f:
                    f.write(json.dumps(stats, indent=2) + '\n')
            if trace and 'w' in trace and fname:      # snapshots only with a batch of one (:292-295)
                base = os.path.splitext(os.path.basename(str(fname[0])))[0]
                tw, ti = trace['w'].cpu().numpy(), trace['img'].cpu().numpy()
                w_in = trace.get('w_in')
                for e in range(self.num_epochs):
                    # w_<name>_<e>.pkl: the reference passes the loop's INPUT latent `w` to snap_w (:292, :636), so its file holds
                    # the same array at every epoch; mirrored.  The latent after this epoch's update goes to w_opt_<name>_<e>.pkl.
                    with open(os.path.join(self.save_dir, f'w_{base}_{e}.pkl'), 'wb') as f:
                        pickle.dump((w_in if w_in is not None else tw[e]).squeeze(), f, pickle.HIGHEST_PROTOCOL)
                    with open(os.path.join(self.save_dir, f'w_opt_{base}_{e}.pkl'), 'wb') as f:
                        pickle.dump(tw[e].squeeze(), f, pickle.HIGHEST_PROTOCOL)
                    if ti.shape[2] >= 2:
                        row = np.concatenate([ti[e, 0, 0], ti[e, 0, 1]], axis=1)      # modality A | modality B
                    else:
                        row = ti[e, 0, 0]
                    row = ((np.clip(row, -1.0, 1.0) + 1) / 2 * 255.0).astype(np.uint8)
                    write_png_gray(os.path.join(self.save_dir, f'{base}_{e}.png'), row)

    def forward(self, w, fname=None, final_noises=None):
        """LatentAug.forward(w, fname) (reference :207-310): returns (imgAB_aug, w_aug) for the FULL batch.

        With an initialised process group every rank passes the same full-batch `w`; rank k optimises samples
        [k*b, (k+1)*b) and a single all_gather returns the whole batch everywhere."""
        if w.ndim == 2:
            w = self.z_to_w(w)                      # reference :209-210
        # crop position: drawn once per forward on the host as the reference does (:216); only the (future) LPIPS
        # criterion consumes it, but the draw is kept so the python RNG stream matches the reference's.
        self.crop_params = get_params(self.res, self.crop_size, self.preprocess)
        import torch.distributed as dist
        if sharded(self.group):
            B = w.shape[0]
            rank = dist.get_rank(self.group)
            lo, hi, per = shard_bounds(B, dist.get_world_size(self.group), rank)
            # The reference draws ONE crop position per forward for the whole batch (:216) and one noise stream for the final
            # synthesis: rank 0's draws are the batch's (control plane: one tiny host-side broadcast of 3 integers; the data
            # path still has exactly one collective).  The final noise is a function of (seed, layer, global batch) only and a rank
            # takes its rows of it, so the gathered batch does not depend on how it was sharded.
            cx, cy, noise_seed = broadcast_controls(self.crop_params['crop_pos'], self.group, self.device, self._host_group())
            self._last_controls = (cx, cy, noise_seed)
            self.crop_params = {'crop_pos': (cx, cy)}
            timers = getattr(self, 'shard_timers', None)      # bench.py: [(start, loop done, gather done)] HIP events per forward
            ev = tuple(torch.cuda.Event(enable_timing=True) for _ in range(3)) if timers is not None else None
            if ev is not None:
                ev[0].record()
                timers.append(ev)      # ([1] and [2] are recorded around the collective, _gather_pair)
            if hi > lo:
                fn = self._shard_noises(final_noises, B, lo, hi, noise_seed)
                if self._verbose_flag and rank == 0:
                    # first-batch log of the reference (:278-300): rank 0 reports its own shard, as replica 0 of a DataParallel run would
                    img, w_aug = self._run_verbose(w[lo:hi], fn, fname[lo:hi] if fname is not None else None)
                else:
                    img, w_aug, _ = self.run_batch(w[lo:hi], fn)
                self._verbose_flag = False
            else:
                img, w_aug = self._empty_pair(0)
            return self._gather_pair(img, w_aug, per, B, ev)
        if self._verbose_flag:
            img, w_aug = self._run_verbose(w, final_noises, fname)
            self._verbose_flag = False
            return img, w_aug
        img, w_aug, _ = self.run_batch(w, final_noises)
        return img, w_aug

    def _run_verbose(self, w, final_noises, fname):
        """One batch with the reference's first-batch artefacts (:278-300): loss scalars of every epoch, and with a batch of one the
        per-epoch snapshots."""
        import time
        trace = {} if w.shape[0] == 1 else None
        lib = _lib.load()
        torch.cuda.synchronize(self.device)
        _lib.check(lib.la_latent_opt_set_time_trace(self._h, 1), 'la_latent_opt_set_time_trace')
        t0 = time.time()
        try:
            img, w_aug, losses = self.run_local(w, final_noises, want_losses=True, trace=trace)
            torch.cuda.synchronize(self.device)
            elapsed = time.time() - t0
            times = None
            if self.num_epochs > 0:      # per-criterion device times of every epoch (the reference's time_* keys, :221-272)
                buf = (C.c_float * (5 * self.num_epochs))()
                _lib.check(lib.la_latent_opt_get_times(self._h, buf), 'la_latent_opt_get_times')
                times = np.asarray(buf, dtype=np.float64).reshape(self.num_epochs, 5) * 1e-3
        finally:
            _lib.check(lib.la_latent_opt_set_time_trace(self._h, 0), 'la_latent_opt_set_time_trace')
        if trace is not None:
            trace['w_in'] = w.detach().cpu().numpy()
        self._log_first_batch(losses, elapsed, trace, fname, times)
        return img, w_aug

    def _host_group(self):
        if self._ctl_group is None:      # once; False = none
            self._ctl_group = host_control_group(self.group, self.device) or False
        return self._ctl_group or None

    @property
    def graph_state(self):
        """1: the optimisation step is replayed from a captured hipGraph; 0: eager launches (`opt.hip_graph = False`, or no batch has
        run yet); -1: eager because the runtime refused the capture.  (With stream lanes: of the lanes, which run the batches.)"""
        if self.lanes_active and self._lanes:
            return min(l.graph_state for l in self._lanes)
        return self._loop.graph_state

    __call__ = forward

    @property
    def mapping(self):
        if self._mapping is None:
            self._mapping = MappingEngine(self._generator, self.device)
            self.z_dim = self._mapping.z_dim
        return self._mapping

    def z_to_w(self, z):
        """reference :459-464: w = reverse_broadcasting(G.mapping(z, None, truncation_psi)); in W+ the mapping's per-row output."""
        ws = self.mapping.forward(z.to(self.device), self.num_ws, self.truncation_psi)
        return ws if self.wplus else self.reverse_broadcasting(ws)

    def forward_ganrand(self, z, noises=None):
        """reference :202-205: w_aug = G.mapping(z, c=None, truncation_psi); img = G.synthesis(w_aug)  (rand_aug mode)."""
        import torch.distributed as dist
        if sharded(self.group):
            # rand_aug with a process group: per-rank capacity is the shard (constructor), so the batch is sharded exactly as in
            # forward() -- rank 0's z is the batch's (the reference draws it once on the host, latent_aug.py:306-308), rank k maps and
            # synthesises samples [k*b, (k+1)*b), ONE all_gather returns image + latent to every rank
            B = z.shape[0]
            rank = dist.get_rank(self.group)
            lo, hi, per = shard_bounds(B, dist.get_world_size(self.group), rank)
            _, _, noise_seed = broadcast_controls((0, 0), self.group, self.device, self._host_group())
            gloo = dist.get_backend(self.group) == 'gloo'
            zb = z.detach().to('cpu' if gloo else self.device, torch.float32).contiguous()
            dist.broadcast(zb, src=dist.get_global_rank(self.group, 0) if self.group is not None else 0, group=self.group)
            if hi > lo:
                ws = self.mapping.forward(zb[lo:hi].to(self.device), self.num_ws, self.truncation_psi)
                img = self.engine.forward(ws, noise_mode=self.final_noise_mode, noises=self._shard_noises(noises, B, lo, hi, noise_seed))
            else:
                img, ws = self._empty_pair(0)
            return self._gather_pair(img, ws, per, B)
        ws = self.mapping.forward(z.to(self.device), self.num_ws, self.truncation_psi)
        img = self.engine.forward(ws, noise_mode=self.final_noise_mode, noises=noises)
        return img, ws


def define_latentaugment(module_name, phase, opt, save_dir, gpu_ids=[], **inject):
    """util_latent_aug.define_latentaugment (reference :45-64) -- returns the module itself (no DataParallel)."""
    if module_name == 'latent_aug':
        return LatentAug(phase, opt, save_dir, gpu_ids, **inject)
    raise NotImplementedError('Module name [%s] is not recognized' % module_name)
