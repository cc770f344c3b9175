"""HBM-resident feature store: the precomputed bottom-up features of a whole dataset fit in one
MI355X's memory (COCO: 123 287 images x 36 x 2048 fp32 = 36 GB of 288 GB), so every image is decompressed and copied to the
device ONCE, the first time it is drawn; from the second epoch on a batch is a device-side row gather (one launch, 2.9 MB at
bs10) and the host only assembles labels.  The reference re-reads, re-decompresses and re-uploads every image every epoch
(`captioning/data/dataloader.py:182-260`, `tools/train.py:178-181`): ~0.3 MB of zlib per image, i.e. a few CPU cores per GPU just
to keep up with a 5 ms SCST iteration.

Wraps a ``FeatureLoader`` and keeps its batch contract; ``fc_feats`` / ``att_feats`` / ``att_masks`` come back as DEVICE tensors
(``DevicePrefetcher`` passes them through), everything else as the wrapped loader returns it.  Images beyond ``budget_bytes`` are
streamed like before.  Storage is ragged ([rows, F] + per-image (offset, K)), so adaptive 10..100-region features cost what
they hold; row 0 is a zero row used as padding.

``norm_att_feat`` and ``use_box`` / ``norm_box_feat`` of a store on a HIP device are applied by the device: the decode pool hands
over the rows as the files hold them, one host-to-device copy carries the rows, the boxes and the per-image table of all newly
drawn images, and one launch of ``capmi_region_rows_build`` (csrc/region_rows.hip) normalises, appends the five geometry columns
and writes every image's rows into the store in the reference's order (by the last column, descending, stable).  The host does
no arithmetic per row; streamed images (beyond the budget) and a store on the CPU keep the loader's numpy path.  ``norm_att_feat`` is
applied to the staged rows first, by ``capmi_rows_l2norm`` (csrc/resident.hip), which sums a row's squares in numpy's order: the store holds
the bits ``finish_image`` gives on the host.

``dtype`` ('fp32', 'bf16', 'fp16'; --resident_dtype) is the element format of the region rows in the store.  The 16-bit formats hold
twice the rows in the same budget: an insert is uploaded or built in fp32 as before, into a staging block of just the new rows, and
``capmi_rows_narrow`` (csrc/resident.hip) rounds the block into the store, to nearest even -- once; a batch widens the stored bits
exactly.  ``fc`` stays fp32 (one row per image), and the mean-of-rows stand-in for a missing fc file is taken from the fp32 rows.

On a HIP device a batch is ONE launch for every dtype: the per-image (first row, K) table goes up as one pinned [B, 2] int32 copy and
``capmi_resident_gather`` writes the widened rows, the zero padding and the mask.  A store on the CPU keeps the torch path
(``.to(dtype)`` on insert, ``.float()`` after ``index_select``).
"""
import numpy as np
import torch

DTYPES = {'fp32': torch.float32, 'bf16': torch.bfloat16, 'fp16': torch.float16}


def check_dtype(name):
    """the start-up check of --resident_dtype (tools/train.py, tools/eval.py, opts.parse_opt)"""
    if name not in DTYPES:
        raise ValueError("resident_dtype %r: the resident store keeps its rows as one of 'fp32', 'bf16', 'fp16'" % (name,))
    return name


class ResidentFeatures:
    def __init__(self, loader, device, budget_bytes=None, first_rows=1 << 16, dtype='fp32'):
        self.loader, self.dev = loader, torch.device(device)
        self.dtype = DTYPES[check_dtype(dtype)]
        self.itemsize = 4 if dtype == 'fp32' else 2
        if budget_bytes is None:
            total = torch.cuda.get_device_properties(self.dev).total_memory if self.dev.type == 'cuda' else 8 << 30
            budget_bytes = total // 2
        self.budget_bytes = int(budget_bytes)
        self.first_rows = int(first_rows)
        self.rows = None               # [capacity, F] of self.dtype; row 0 stays zero
        self.fc = None                 # [n_images, F_fc]
        self.used = 1
        self.slot = {}                 # image index -> (first row, K)
        self.n_images = len(loader.info['images'])
        self._pending = {}
        self.hits = self.misses = self.streamed = 0
        # rows built by the device from raw files (module docstring); otherwise the loader's decode has already finished them
        self.device_build = self.dev.type == 'cuda' and bool(getattr(loader, 'norm_att_feat', False) or getattr(loader, 'use_box', False))

    def __getattr__(self, name):       # vocabulary, pos, order, document_frequency(), ... of the wrapped loader
        return getattr(self.loader, name)

    # ---- storage
    def _room(self, k, F):
        """make room for k more rows; False when the budget does not allow it"""
        if self.rows is None:
            cap = max(self.first_rows, 2 * k + 1)
            if cap * F * self.itemsize > self.budget_bytes:
                cap = self.budget_bytes // (F * self.itemsize)
            if cap < k + 1:
                return False
            self.rows = torch.zeros(cap, F, dtype=self.dtype, device=self.dev)
            return True
        if self.used + k <= self.rows.shape[0]:
            return True
        cap = min(max(2 * self.rows.shape[0], self.used + k), self.budget_bytes // (F * self.itemsize))
        if cap < self.used + k:
            return False
        grown = torch.zeros(cap, F, dtype=self.dtype, device=self.dev)
        grown[:self.used].copy_(self.rows[:self.used])
        self.rows = grown
        return True

    def _build_many(self, new):
        """_insert_many for raw images [(ix, fc or None, att as in the file, boxes or None)]: one copy (rows | boxes | table), one
        launch into self.rows (a 16-bit store: into an fp32 block of the new rows, which capmi_rows_narrow rounds into self.rows); the
        ones that did not fit come back finished by the loader's host path as (ix, fc, att)"""
        from imagecaptioning.pytorch_amd import ops
        ld = self.loader
        box = bool(ld.use_box)
        fit, loose, k_tot = [], [], 0
        for ix, fc, att, boxes in new:
            if self._room(k_tot + att.shape[0], att.shape[1] + 5 * box):
                fit.append((ix, fc, att, boxes))
                k_tot += att.shape[0]
            else:
                loose.append((ix,) + ld.finish_image(ix, fc, att, boxes))
        if fit:
            D = fit[0][2].shape[1]
            table = np.zeros((len(fit), 4), dtype=np.int32)
            r = 0
            for i, (ix, _, att, _) in enumerate(fit):
                im = ld.info['images'][ix]
                table[i] = (r, att.shape[0], int(im['height']), int(im['width'])) if box else (r, att.shape[0], 0, 0)
                r += att.shape[0]
            pad = lambda n: (n + 3) & ~3                           # noqa: E731  (every part starts on 16 bytes)
            o_box = pad(k_tot * D)
            o_tab = o_box + pad(k_tot * 4 * box)
            host = np.zeros(o_tab + table.size, dtype=np.float32)
            host[:k_tot * D] = np.concatenate([a for _, _, a, _ in fit], 0).reshape(-1)
            if box:
                host[o_box:o_box + k_tot * 4] = np.concatenate([b for _, _, _, b in fit], 0).reshape(-1)
            host[o_tab:].view(np.int32)[:] = table.reshape(-1)
            stage = torch.from_numpy(host).to(self.dev)
            F = self.rows.shape[1]
            place = self.rows[self.used:self.used + k_tot]
            built = place if self.itemsize == 4 else torch.empty(k_tot, F, dtype=torch.float32, device=self.dev)
            raw = stage[:k_tot * D].view(k_tot, D)
            if ld.norm_att_feat:                                   # in numpy's summation order: the bits of finish_image on the host
                ops.rows_l2norm(raw)
            ops.region_rows_build(raw, stage[o_box:o_box + k_tot * 4].view(k_tot, 4) if box else None,
                                  table, stage[o_tab:].view(torch.int32), built, False, box, ld.norm_box_feat)
            if built is not place:
                ops.rows_narrow(built, place)
            if self.fc is None:
                self.fc = torch.zeros(self.n_images, F if fit[0][1] is None else fit[0][1].shape[0], dtype=torch.float32, device=self.dev)
            if self.fc.shape[1]:
                ixs = torch.tensor([ix for ix, _, _, _ in fit], dtype=torch.int64).to(self.dev)
                zero = np.zeros(self.fc.shape[1], dtype=np.float32)
                self.fc.index_copy_(0, ixs, torch.from_numpy(np.stack([zero if f is None else f for _, f, _, _ in fit])).to(self.dev))
            r = 0
            for ix, fc, att, _ in fit:
                self.slot[ix] = (self.used, att.shape[0])
                if fc is None and self.fc.shape[1]:                # no fc file: the mean of the built rows (dataloader.py:295-298)
                    self.fc[ix] = built[r:r + att.shape[0]].mean(0)
                self.used += att.shape[0]
                r += att.shape[0]
        return loose

    def _insert_many(self, new):
        """new: [(ix, fc, att)] -> the ones that did not fit; ONE host-to-device copy for all region rows, one for the fc rows"""
        if self.device_build:
            return self._build_many(new)
        fit, loose, k_tot = [], [], 0
        for ix, fc, att in new:
            if self._room(k_tot + att.shape[0], att.shape[1]):
                fit.append((ix, fc, att))
                k_tot += att.shape[0]
            else:
                loose.append((ix, fc, att))
        if fit:
            block = torch.from_numpy(np.concatenate([a for _, _, a in fit], 0))
            place = self.rows[self.used:self.used + k_tot]
            if self.itemsize == 4:
                place.copy_(block)
            elif self.dev.type == 'cuda':                          # one fp32 copy up, rounded into the store by the device
                from imagecaptioning.pytorch_amd import ops
                ops.rows_narrow(block.to(self.dev), place)
            else:
                place.copy_(block.to(self.dtype))
            if self.fc is None:
                self.fc = torch.zeros(self.n_images, fit[0][1].shape[0], dtype=torch.float32, device=self.dev)
            if self.fc.shape[1]:
                ixs = torch.tensor([ix for ix, _, _ in fit], dtype=torch.int64).to(self.dev)
                self.fc.index_copy_(0, ixs, torch.from_numpy(np.stack([f for _, f, _ in fit])).to(self.dev))
            for ix, _, att in fit:
                self.slot[ix] = (self.used, att.shape[0])
                self.used += att.shape[0]
        return loose

    @property
    def resident_bytes(self):
        return 0 if self.rows is None else self.used * self.rows.shape[1] * self.itemsize

    def reset_iterator(self, split):
        """DataLoader.reset_iterator (dataloader.py:356-358): drop what was scheduled ahead, start the split over"""
        for key in [k for k in self._pending if k[0] == split]:
            self._pending.pop(key)
        self.loader.reset_iterator(split)

    # ---- batches
    def _schedule(self, split, B):
        idx, wrapped = self.loader._next_indices(split, B)
        raw = (True,) if self.device_build else ()
        futs = {ix: self.loader.submit_image(ix, *raw) for ix in set(idx) if ix not in self.slot}
        return idx, wrapped, self.loader.pos[split], futs, self.loader._snap[split], self.loader.rng.getstate()

    def get_batch(self, split, batch_size=None):
        ld = self.loader
        B = batch_size or ld.batch_size
        key = (split, B)
        q = self._pending.setdefault(key, [])
        while len(q) < ld.lookahead + 1:                       # decode the NEXT batches' new images in the background
            q.append(self._schedule(split, B))
        idx, wrapped, pos_now, futs, snap, rng_state = q.pop(0)
        B = len(idx)                                           # (the last batch of a val / test pass may be short)
        new, seen = [], set()
        for ix in idx:
            if ix in self.slot:
                self.hits += 1
            elif ix not in seen:
                seen.add(ix)
                new.append((ix,) + tuple(futs[ix].result() if ix in futs else ld._image(ix, *((True,) if self.device_build else ()))))
                self.misses += 1
        loose = {ix: (fc, att) for ix, fc, att in self._insert_many(new)}      # images the budget has no room for: streamed
        self.streamed += len(loose)
        ks = [self.slot[ix][1] if ix in self.slot else loose[ix][1].shape[0] for ix in idx]
        kmax = max(ks)
        F = self.rows.shape[1] if self.rows is not None else next(iter(loose.values()))[1].shape[1]
        att_masks = None
        if self.rows is not None and self.dev.type == 'cuda':  # one table up, one launch: rows widened, padding zeroed, mask written
            from imagecaptioning.pytorch_amd import ops
            pinned = torch.zeros(B, 2, dtype=torch.int32, pin_memory=True)
            table = pinned.numpy()
            for b, ix in enumerate(idx):
                if ix in self.slot:
                    table[b] = self.slot[ix]
            att, att_masks = ops.resident_gather(self.rows, table, pinned.to(self.dev, non_blocking=True), kmax)
        elif self.rows is not None:
            gather = np.zeros((B, kmax), dtype=np.int64)       # 0 = the zero row
            for b, ix in enumerate(idx):
                if ix in self.slot:
                    r0, k = self.slot[ix]
                    gather[b, :k] = np.arange(r0, r0 + k)
            att = self.rows.index_select(0, torch.from_numpy(gather.reshape(-1)).to(self.dev)).float().view(B, kmax, F)
        else:
            att = torch.zeros(B, kmax, F, dtype=torch.float32, device=self.dev)
        ix_t = torch.tensor(idx, dtype=torch.int64).to(self.dev)
        fc = self.fc.index_select(0, ix_t) if self.fc is not None else None
        for b, ix in enumerate(idx):
            if ix in loose:
                f, a = loose[ix]
                att[b, :a.shape[0]].copy_(torch.from_numpy(np.ascontiguousarray(a)))
                if fc is None:
                    fc = torch.zeros(B, f.shape[0], dtype=torch.float32, device=self.dev)
                if f.shape[0]:
                    fc[b].copy_(torch.from_numpy(np.ascontiguousarray(f)))
        if min(ks) == kmax:                                    # dataloader.py:240-241: None when every image fills kmax regions
            att_masks = None
        elif att_masks is None:
            m = np.zeros((B, kmax), dtype=np.float32)
            for b, k in enumerate(ks):
                m[b, :k] = 1
            att_masks = torch.from_numpy(m).to(self.dev)
        else:                                                  # the launch knows the resident images; the streamed ones' K is known here
            for b, ix in enumerate(idx):
                if ix in loose:
                    att_masks[b, :ks[b]] = 1
        if att_masks is not None:
            att_masks._capmi_kmax = kmax   # clip_att's K (ops.clip_len): no device->host sync in the step
        labels, masks, gts, infos = ld.label_part(idx)
        state = {'loader_order': {split: snap}, 'loader_rng': rng_state, 'loader_cap_rng': ld.cap_rng.getstate()}
        return {'fc_feats': fc, 'att_feats': att, 'att_masks': att_masks, 'labels': torch.from_numpy(labels),
                'masks': torch.from_numpy(masks), 'gts': gts,
                'bounds': {'it_pos_now': pos_now, 'it_max': len(ld.order[split]), 'wrapped': wrapped, 'loader_state': state},
                'infos': infos}
