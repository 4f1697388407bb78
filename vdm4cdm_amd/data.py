"""Synthetic CAMELS-like data module emitting the reference's batch-dict contract.

The reference's ``AstroDataModule`` (/root/reference/src/dataset/CAMELS_3D_dataset.py:76-198) reads 1000 x D^3 cubes
from a Harvard cluster path; that I/O layer is out of scope.  What the hot path consumes is
its batch dict, built by the scripts' ``return_func`` (/root/reference/trainVDM3D128_c_c_from_field_name_thick_lowbatch.py:75-76):

    {"conditioning": (B,1,D,D,D), "x": (B,1,D,D,D), "conditioning_values": [(B,6)]}

and its ``norm_func`` / ``unnorm_func`` pair (CAMELS_3D_dataset.py:146-156): x = (log10(rho + alpha) - m) / s.
This module produces that dict from seeded synthetic fields: the target is a unit-variance Gaussian
random field with P(k) ~ k^-2 in normalised-log-density space (== a lognormal density cube), the conditioning
field is the standardised ``relu(g - 1)`` of the same field (sparse, stellar-mass-like), the six parameters are
uniform in the CAMELS ranges.

``AstroDataModule`` is the file-backed module with the reference's constructor and loader surface, re-designed for the GPU
(SURVEY.md section 8f rank 3): the raw ``.npy`` cube stacks are uploaded to HBM ONCE (the 128^3 LH set is 8 GB per field, the
256^3 set 67 GB - of 288 GB), and every batch is produced by ONE HIP launch (``vdm_augment_batch``: periodic crop at a shifted
anchor, log10 + normalisation, flips, axis permutation) instead of 16 CPU DataLoader workers.  Only the integer choices (which
simulation / crop, shift, flips, permutation) are drawn on the host.
"""
import math
import os
import warnings

import numpy as np
import torch

# field -> (mean, std, alpha) of log10(rho + alpha)   [/root/reference/src/dataset/normalizations_3d.json:2-5, alphas_3d.json:2-3]
FIELD_NORM = {"Mcdm": (10.019186, 0.552020, 1.0), "Mstar": (0.010429, 0.321929, 1.0)}
PARAM_LO = torch.tensor([0.1, 0.6, 0.25, 0.25, 0.5, 0.5])
PARAM_HI = torch.tensor([0.5, 1.0, 4.0, 4.0, 2.0, 2.0])


def gaussian_random_field(shape, generator=None, slope=-2.0, device="cpu"):
    """Unit-variance GRF with P(k) ~ k^slope over the trailing spatial dims of `shape` = (B, C, *spatial)."""
    nd = len(shape) - 2
    dims = tuple(range(2, 2 + nd))
    w = torch.randn(shape, generator=generator, device=device)
    Fw = torch.fft.fftn(w, dim=dims)
    ks = torch.meshgrid(*[torch.fft.fftfreq(n, device=device) * n for n in shape[2:]], indexing="ij")
    k = torch.sqrt(sum(kk ** 2 for kk in ks))
    amp = torch.where(k > 0, k.clamp(min=1.0) ** (slope / 2.0), torch.zeros_like(k))
    x = torch.fft.ifftn(Fw * amp, dim=dims).real
    x = x - x.mean(dim=dims, keepdim=True)
    return (x / x.std(dim=dims, keepdim=True)).float()


MAX_COND_FIELDS = 3          # conditioning fields the HIP CUNet takes at once (conv_in's input stays one 16-byte piece per voxel)


def split_fields(field_in):
    """"A", "A+B" or "A+B+C" (the <field_in> of the training scripts, `in_field_name` of a config) -> the list of conditioning field
    names.  ValueError for an empty name, a repeated field or more than MAX_COND_FIELDS fields."""
    names = str(field_in).split("+")
    if any(not n.strip() for n in names):
        raise ValueError(f"conditioning fields {field_in!r}: empty field name")
    names = [n.strip() for n in names]
    if len(set(names)) != len(names):
        raise ValueError(f"conditioning fields {field_in!r}: a field is repeated")
    if len(names) > MAX_COND_FIELDS:
        raise ValueError(f"conditioning fields {field_in!r}: at most {MAX_COND_FIELDS} fields at once, got {len(names)}")
    return names


def cond_return_func(n_cond, values=True):
    """return_func(fields, params) of a conditional model on fields = [c_0, .., c_{K-1}, x]: conditioning [B, K, ...] (the K fields
    concatenated on the channel axis), x = the last field.  The channel axis is the fourth from the end of a 3D field: the file-backed
    module calls this per sample ([1, D, H, W] fields), the synthetic module per batch ([B, 1, D, H, W])."""
    def return_func(fields, params):
        cond = fields[0] if n_cond == 1 else torch.cat(list(fields[:n_cond]), dim=-4)
        return {"conditioning": cond, "x": fields[n_cond], "conditioning_values": [params] if values else None}
    return return_func


class SyntheticAstroDataModule:
    """Same surface as the reference DataModule as far as the hot path and the scripts touch it.  len(channel_names) - 1 conditioning
    fields (at least one): field j is the thresholded target relu(x - (1.0 - 0.5 j)), standardised - correlated with x and with each
    other, but distinct; fields = [c_0, .., c_{K-1}, x]."""

    def __init__(self, cropsize=128, batch_size=2, dim=3, n_train=950, n_val=50, n_test=12, channel_names=("Mstar", "Mcdm"),
                 conditioning=True, n_params=6, seed=1000, device="cpu", return_func=None, pool=8):
        self.cropsize, self.batch_size, self.dim = cropsize, batch_size, dim
        self.n_train, self.n_val, self.n_test = n_train, n_val, n_test
        self.channel_names = list(channel_names)
        self.conditioning, self.n_params = conditioning, n_params
        self.seed, self.device = seed, device
        self.return_func = return_func
        self.pool = pool                      # number of distinct cached batches (generation is not the hot path)
        self._cache = {}

    # -- normalisation pair (CAMELS_3D_dataset.py:146-156) --------------------------------------------
    def _norm_consts(self, i_channel):
        return FIELD_NORM.get(self.channel_names[i_channel], (0.0, 1.0, 1.0))

    def norm_func(self, x, i_channel):
        m, s, a = self._norm_consts(i_channel)
        return (torch.log10(x + a) - m) / s

    def unnorm_func(self, x, i_channel):
        m, s, a = self._norm_consts(i_channel)
        return 10 ** (x * s + m) - a

    # -- batches -------------------------------------------------------------------------------------
    def _make_batch(self, seed, batch_size):
        g = torch.Generator().manual_seed(seed)
        shape = (batch_size, 1) + (self.cropsize,) * self.dim
        x = gaussian_random_field(shape, generator=g)
        params = PARAM_LO + (PARAM_HI - PARAM_LO) * torch.rand(batch_size, 6, generator=g)
        cond, conds = None, [None]
        if self.conditioning:
            dims = tuple(range(2, 2 + self.dim))
            conds = []
            for j in range(max(1, len(self.channel_names) - 1)):
                c = torch.relu(x - (1.0 - 0.5 * j))
                c = c - c.mean(dim=dims, keepdim=True)
                conds.append(c / c.std(dim=dims, keepdim=True).clamp(min=1e-6))
            cond = conds[0] if len(conds) == 1 else torch.cat(conds, dim=1)
        fields = conds + [x]
        if self.return_func is not None:
            batch = self.return_func(fields, params[:, :self.n_params])
        else:
            batch = {"conditioning": cond, "x": x, "conditioning_values": [params[:, :self.n_params]] if self.n_params else []}
        return batch

    def _loader(self, base_seed, n_items, batch_size, rank=0, world=1, start_batch=0):
        n_batches = max(1, n_items // (batch_size * world))
        for b in range(start_batch, n_batches):
            key = (base_seed, (b * world + rank) % self.pool, batch_size)
            if key not in self._cache:
                self._cache[key] = self._make_batch(base_seed + key[1], batch_size)
            batch = self._cache[key]
            yield {k: (self._to(v)) for k, v in batch.items()}

    def _to(self, v):
        if v is None:
            return None
        if isinstance(v, (list, tuple)):
            return [a.to(self.device, non_blocking=True) for a in v]
        return v.to(self.device, non_blocking=True)

    def train_dataloader(self, rank=0, world=1, start_batch=0):
        """start_batch: begin at that batch of the epoch (a resumed run; the batches are a pure function of their index)."""
        return self._loader(self.seed + 7919 * rank, self.n_train, self.batch_size, rank, world, start_batch)

    def state_dict(self):
        """What identifies the batch sequence (the position inside the epoch is the trainer's `batches_into_epoch`)."""
        return {"kind": type(self).__name__, "seed": int(self.seed), "n_train": int(self.n_train), "batch_size": int(self.batch_size),
                "cropsize": int(self.cropsize), "dim": int(self.dim), "pool": int(self.pool)}

    def load_state_dict(self, state):
        _check_same_module(self.state_dict(), state)

    def val_dataloader(self, rank=0, world=1):
        return self._loader(self.seed + 500000, self.n_val, self.batch_size, rank, world)

    def test_dataloader(self, rank=0, world=1):
        return self._loader(self.seed + 900000, self.n_test, self.batch_size, rank, world)


# field -> alpha of log10(rho + alpha)  [/root/reference/src/dataset/alphas_3d.json]; (mean, std) [normalizations_3d.json]
ALPHAS = {"Mcdm": 1.0, "Mstar": 1.0, "B": 1.0, "HI": 1.0, "Mgas": 1.0, "MgFe": 1.0, "ne": 1.0, "P": 1.0, "T": 1.0, "Z": 1.0,
          "Go7": 2.0, "Go8": 2.0, "Go9": 2.0}
NORMALIZATIONS = {"Mcdm": (10.019186475678042, 0.5520203178284999), "Mstar": (0.010429391444558287, 0.3219291117577123),
                  "Go7": (0.0, 1.0), "Go8": (0.0, 1.0), "Go9": (0.0, 1.0)}
DATA_ROOT_ENV = "VDM4CDM_DATA_ROOT"
# "1": a missing 3D_grids_<S> set is derived in HBM from the 256^3 stack (trilinear, as make_down_grids writes it) instead of failing
DOWNGRID_ENV = "VDM4CDM_DOWNGRID"
# a JSON file in the reference's flat schema {"<field>_m": mean, "<field>_s": std} (calc_normalization.py writes it): the constants of the
# fields it names replace / extend NORMALIZATIONS in every AstroDataModule
NORMALIZATIONS_ENV = "VDM4CDM_NORMALIZATIONS"


def grid_size(dataset_name):
    """"CMD" -> 256, "CMD_128" -> 128, ... (the key scheme of /root/reference/src/dataset/data_source_3d.json)."""
    return 256 if dataset_name == "CMD" else int(dataset_name.split("_")[1])


def field_path(root, dataset_name, suite_name, set_name, z_name, channel_name):
    """File layout of the CAMELS grids below the cluster directory the reference reads
    (/root/reference/src/dataset/data_source_3d.json: .../Camels/3D_grids_new/Grids_Mcdm_Astrid_LH_256_z=0.0.npy,
    .../Camels/3D_grids_128/Grids_Mstar_Astrid_CV_128_z=0.0.npy), relative to `root`."""
    S = grid_size(dataset_name)
    sub = "3D_grids_new" if S == 256 else f"3D_grids_{S}"
    z = z_name.split("_", 1)[1]
    return os.path.join(root, sub, f"Grids_{channel_name}_{suite_name}_{set_name}_{S}_z={z}.npy")


def down_grid_edge(nside, s_file):
    """Edge T of the down-gridded cubes of data set CMD_<nside> made from a "256" stack whose cubes really have edge `s_file`:
    T = nside * s_file / 256 (CAMELS: s_file == 256, T == nside; a small stand-in stack keeps the ratio).  ValueError unless 1 <=
    nside <= 256 and T is an integer."""
    if isinstance(nside, bool) or not isinstance(nside, (int, np.integer)) or not 1 <= nside <= 256:
        raise ValueError(f"down-gridding: nside = {nside!r} must be an integer in 1..256")
    if (int(nside) * int(s_file)) % 256:
        raise ValueError(f"down-gridding: nside = {nside} of a source stack with edge {s_file} gives the non-integer edge "
                         f"{nside * s_file / 256:g} (T = nside * edge / 256)")
    return int(nside) * int(s_file) // 256


def _slab_sims(f):
    """Whole simulations per upload slab: at most 1 GiB of the stack `f`, at least one cube."""
    return max(1, (1 << 30) // max(1, f[0].nbytes))


def load_normalizations(path):
    """{field: (mean, std)} of a normalisation file in the reference's flat schema {"<field>_m": ..., "<field>_s": ...}
    (the reference's src/dataset/normalizations_3d.json).  ValueError for a file that cannot be read, is not a flat object of numbers,
    names one of a field's two constants without the other, or holds a non-finite value or a std <= 0."""
    import json
    try:
        with open(path) as fh:
            raw = json.load(fh)
    except (OSError, ValueError) as e:
        raise ValueError(f"normalisation file {path!r} cannot be read: {e}") from None
    if not isinstance(raw, dict):
        raise ValueError(f"normalisation file {path!r} holds a {type(raw).__name__}, not a flat object {{\"<field>_m\": mean, \"<field>_s\": std}}")
    out = {}
    for key, v in raw.items():
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise ValueError(f"normalisation file {path!r}: {key!r} is {v!r}, not a number (the file is a flat object of numbers)")
        if key[-2:] not in ("_m", "_s") or len(key) < 3:
            raise ValueError(f"normalisation file {path!r}: key {key!r} is neither \"<field>_m\" nor \"<field>_s\"")
        if not math.isfinite(v):
            raise ValueError(f"normalisation file {path!r}: {key!r} = {v!r} is not finite")
        out.setdefault(key[:-2], {})[key[-1]] = float(v)
    for field, c in out.items():
        if len(c) != 2:
            have, miss = ("_m", "_s") if "m" in c else ("_s", "_m")
            raise ValueError(f"normalisation file {path!r} names {field + have!r} without {field + miss!r}")
        if c["s"] <= 0:
            raise ValueError(f"normalisation file {path!r}: {field + '_s'!r} = {c['s']!r} must be positive")
    return {field: (c["m"], c["s"]) for field, c in out.items()}


def params_path(root, suite_name, set_name):
    """.../Camels/params_new/params_{set}_{suite}.txt (/root/reference/src/dataset/CAMELS_3D_dataset.py:123)."""
    return os.path.join(root, "params_new", f"params_{set_name}_{suite_name}.txt")


def default_return_func(fields, params):
    """/root/reference/src/dataset/CAMELS_3D_dataset.py:217-219."""
    return {"x": torch.cat(fields, dim=0), "conditioning": None, "conditioning_values": params}


class AstroDataModule:
    """File-backed CAMELS module: constructor, ``norm_func`` / ``unnorm_func``, ``collate_fn`` and the three loaders of the
    reference's ``AstroDataModule`` (/root/reference/src/dataset/CAMELS_3D_dataset.py:76-198), with the per-sample work of
    ``AstroDataset.__getitem__`` (:53-73) done by one HIP launch per batch on `device`.

    Differences by design: no worker processes (``num_workers`` is accepted and ignored), batches are born on the GPU, and the
    random anchor shift is drawn fresh around the grid anchor for every sample (the reference adds it IN PLACE to its anchor table,
    augmentation.py:113-117, so its anchors random-walk over the epochs; both are uniform periodic translations)."""

    def __init__(self, selection, channel_names, return_func, stage="fit", batch_size=1, do_crop=False, cropsize=256, ndim=3,
                 num_workers=1, mmap=True, data_root=None, device=None, seed=0):
        assert stage in ["fit", "test"], f"stage {stage} not recognized"
        assert ndim == 3, "the device data path covers the 3D grids (the 2D maps belong to the CPU plumbing config C1)"
        self.ndim, self.selection, self.channel_names = ndim, selection, list(channel_names)
        self.stage, self.batch_size, self.do_crop, self.cropsize = stage, batch_size, do_crop, cropsize
        self.num_workers, self.mmap = num_workers, mmap
        self.return_func = return_func if return_func is not None else default_return_func
        self.device = device
        self.alphas = [ALPHAS[c] for c in self.channel_names]
        norm_file = os.environ.get(NORMALIZATIONS_ENV)
        from_file = load_normalizations(norm_file) if norm_file else {}
        self._norm_from_file = [c in from_file for c in self.channel_names]
        for c in self.channel_names:
            if c in from_file:
                print(f"[data] {c}: normalisation constants mean = {from_file[c][0]!r}, std = {from_file[c][1]!r} from {norm_file} "
                      f"(${NORMALIZATIONS_ENV})", flush=True)
            elif c not in NORMALIZATIONS:
                raise KeyError(f"no normalisation constants for field {c!r}: the built-in table has {sorted(NORMALIZATIONS)}"
                               + (f" and {norm_file} has {sorted(from_file)}" if norm_file else "")
                               + f"; derive them once with `python calc_normalization.py {c}` and point ${NORMALIZATIONS_ENV} at the file it writes")
        consts = [from_file.get(c) or NORMALIZATIONS[c] for c in self.channel_names]
        self.means = [m for m, _ in consts]
        self.stds = [s for _, s in consts]
        root = data_root or os.environ.get(DATA_ROOT_ENV)
        assert root, f"AstroDataModule needs the CAMELS directory (data_root= or ${DATA_ROOT_ENV})"
        sel = selection
        cv = sel["set_name"] == "CV"
        self.fields = []
        self._derived_edge = []                  # per channel: None (the file has the data set's size) or the edge to down-grid to
        for c in self.channel_names:
            # always memory-mapped, whatever `mmap` says (the reference's scripts pass mmap=False and hold the whole set - 67 GB per field at
            # 256^3 - in host RAM, once per rank): here the cubes live in HBM after _resident() uploaded them slab by slab, the host only
            # ever touches one slab
            path = field_path(root, sel["dataset_name"], sel["suite_name"], sel["set_name"], sel["z_name"], c)
            edge = None
            if os.environ.get(DOWNGRID_ENV) == "1" and grid_size(sel["dataset_name"]) != 256 and not os.path.exists(path):
                # opt-in: the resampled set is not on disk - open the 256^3 stack instead; _resident() down-grids every slab it uploads
                src = field_path(root, "CMD", sel["suite_name"], sel["set_name"], sel["z_name"], c)
                if not os.path.exists(src):
                    raise FileNotFoundError(f"{path} does not exist and ${DOWNGRID_ENV}=1 cannot derive it: the 256^3 stack {src} is missing too")
                f = np.load(src, mmap_mode="r")
                edge = down_grid_edge(grid_size(sel["dataset_name"]), f.shape[-1])
                print(f"[data] {c}: {sel['dataset_name']} is derived on the device from {src} (trilinear {f.shape[-1]} -> {edge}, "
                      f"${DOWNGRID_ENV}=1)", flush=True)
            else:
                f = np.load(path, mmap_mode="r")
            self.fields.append(f[_cv_keep(len(f))] if cv else f)
            self._derived_edge.append(edge)
        self.params = np.atleast_2d(np.loadtxt(params_path(root, sel["suite_name"], sel["set_name"]))).astype(np.float32)
        if cv:
            self.params = self.params[_cv_keep(len(self.params))]
        edges = [int(f.shape[-1]) if e is None else e for f, e in zip(self.fields, self._derived_edge)]
        self.fullsize = edges[0]
        for f, e in zip(self.fields, edges):
            assert f.ndim == 4 and f.shape[1:] == (f.shape[-1],) * 3 and e == self.fullsize and len(f) == len(self.fields[0]), \
                "field shapes disagree"
        assert len(self.params) == len(self.fields[0]), f"len(params)={len(self.params)} != len(fields)={len(self.fields[0])}"
        self.crop = cropsize if do_crop else self.fullsize
        ax = np.arange(0, self.fullsize, self.crop)
        self.anchors = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), axis=-1).reshape(-1, 3)      # augmentation.py:97-103
        self.ncrops = len(self.anchors)
        self.nsamples = len(self.fields[0]) * self.ncrops
        # two generators: the epoch shuffles must stay IDENTICAL on every rank (disjoint shards epoch after epoch), the augmentation
        # draws are per rank
        self._seed = int(seed)
        self._gen = torch.Generator().manual_seed(self._seed)                      # split + epoch shuffles (same on all ranks)
        # shifts / flips / permutations: one generator per (training rank), seeded ONCE at its first use and never again, and a
        # separate one for the validation / test loaders - a validation pass must not touch (let alone re-seed) the training stream
        self._aug_gens = {}
        self._aug_gen = self._aug_generator("train", 0)
        if stage == "fit":                                       # random_split(data, [95 %, 5 %])  (CAMELS_3D_dataset.py:134-137)
            order = torch.randperm(self.nsamples, generator=self._gen).tolist()
            n_train = int(self.nsamples * 0.95)
            self.train_idx, self.valid_idx = order[:n_train], order[n_train:]
        else:
            self.test_idx = list(range(self.nsamples))
        self._epoch_gen_state = None                              # _gen's state where the current training epoch drew its order
        self._dev_fields = None

    # -- normalisation pair (CAMELS_3D_dataset.py:146-156) --------------------------------------------
    def unnorm_func(self, field, i_channel):
        return 10 ** (field * self.stds[i_channel] + self.means[i_channel]) - self.alphas[i_channel]

    def norm_func(self, field, i_channel):
        return (torch.log10(field + self.alphas[i_channel]) - self.means[i_channel]) / self.stds[i_channel]

    def collate_fn(self, batch):
        """CAMELS_3D_dataset.py:158-171: tensors are stacked, lists of tensors are stacked entry by entry, None stays None."""
        out, b0 = {}, batch[0]
        for key in b0.keys():
            if b0[key] is None:
                out[key] = None
            elif isinstance(b0[key], torch.Tensor):
                out[key] = torch.stack([b[key] for b in batch], dim=0)
            elif isinstance(b0[key], list):
                out[key] = [torch.stack([b[key][i] for b in batch], dim=0) for i in range(len(b0[key]))]
            else:
                raise ValueError(f"Type of {key} not recognized")
        return out

    # -- batches on the device ------------------------------------------------------------------------
    def _resident(self):
        if self._dev_fields is None:
            dev = torch.device(self.device if self.device is not None else "cuda")
            if dev.type != "cuda":
                raise RuntimeError("AstroDataModule builds its batches with a HIP kernel: set .device to a GPU (there is no CPU path)")
            self._dev_fields = []
            for f, edge in zip(self.fields, self._derived_edge):  # upload in slabs of simulations: the (memory-mapped) 256^3 sets are
                step = _slab_sims(f)                                       # 67 GB per field - never a second full copy on the host
                if edge is None:
                    d = torch.empty(f.shape, dtype=torch.float32, device=dev)
                    for i in range(0, len(f), step):
                        d[i:i + step].copy_(torch.from_numpy(np.ascontiguousarray(f[i:i + step], dtype=np.float32)))
                else:                             # derived set: every slab of the 256^3 stack is down-gridded straight into the resident stack
                    from . import hip_ops as ops
                    d = torch.empty((len(f),) + (edge,) * 3, dtype=torch.float32, device=dev)
                    slab = torch.empty((min(step, len(f)),) + tuple(f.shape[1:]), dtype=torch.float32, device=dev)
                    for i in range(0, len(f), step):
                        k = min(step, len(f) - i)
                        slab[:k].copy_(torch.from_numpy(np.ascontiguousarray(f[i:i + k], dtype=np.float32)))
                        ops.downgrid_trilinear(slab[:k], edge, out=d[i:i + k])
                    del slab
                self._dev_fields.append(d)
            self._dev_params = torch.from_numpy(self.params).to(dev)
        return self._dev_fields

    def _aug_generator(self, kind, rank):
        key = (kind, int(rank))
        g = self._aug_gens.get(key)
        if g is None:
            g = self._aug_gens[key] = torch.Generator().manual_seed(self._seed + 1 + 7919 * int(rank) + (0 if kind == "train" else 104729))
        return g

    def draw_sample(self, idx, train, gen=None):
        """(sim, anchor, flips, perm) of dataset item `idx`: bidx, icrop = divmod(idx, ncrops) (CAMELS_3D_dataset.py:55); in the
        "fit" stage the anchor is shifted by randint(crop) per axis, flips ~ randint(2), perm ~ randperm (augmentation.py:48-49,
        69, 113-117), all from `gen` (default: this module's rank-0 training generator)."""
        gen = self._aug_gen if gen is None else gen
        sim, icrop = divmod(int(idx), self.ncrops)
        anchor = self.anchors[icrop].copy()
        flips, perm = [0, 0, 0], [0, 1, 2]
        if train:
            anchor = anchor + torch.randint(self.crop, (3,), generator=gen).numpy()
            flips = torch.randint(2, (3,), generator=gen).tolist()
            perm = torch.randperm(3, generator=gen).tolist()
        return sim, anchor.tolist(), flips, perm

    def make_batch(self, samples):
        """samples: list of (sim, anchor, flips, perm) -> the collated batch dict (one HIP launch for all samples and channels)."""
        from . import hip_ops as ops
        fields = self._resident()
        consts = list(zip(self.alphas, self.means, self.stds))
        outs = ops.augment_batch(fields, consts, samples, self.crop)
        items = [self.return_func(fields=[o[b] for o in outs], params=self._dev_params[s[0]]) for b, s in enumerate(samples)]
        return self.collate_fn(items)

    def shard(self, idx, rank, world):
        """This rank's items of one epoch order.  world == 1: all of them (the reference's single-process DataLoader, a short last
        batch included).  world > 1: the order is padded by wrap-around to a multiple of world * batch_size and dealt out strided, so
        every rank sees the SAME number of FULL batches (torch's DistributedSampler rule: repeat, never drop) - ranks cannot drift
        across epoch boundaries, and the global time stratification (vdm_model.stratified_times) always sees equal local batches."""
        idx = list(idx)
        if world <= 1 or not idx:
            return idx
        unit = world * self.batch_size
        total = -(-len(idx) // unit) * unit
        idx = (idx * (total // len(idx) + 1))[:total]
        return idx[rank::world]

    def _loader(self, indices, train, shuffle, rank=0, world=1, kind="train", start_batch=0):
        gen = self._aug_generator(kind, rank)                     # (seeded once per (kind, rank); never re-seeded)
        idx = list(indices)
        if shuffle:
            self._epoch_gen_state = self._gen.get_state()
            idx = [idx[i] for i in torch.randperm(len(idx), generator=self._gen).tolist()]
        if kind == "eval" and world > 1:
            # validation / test: every item exactly once over the ranks (strided, NO wrap-around padding: a duplicated item would be
            # over-weighted in val_loss and emitted twice by a sharded test pass); ranks may differ by one item - Trainer.validate
            # weights its one all-reduce by the samples each rank really saw
            idx = idx[rank::world]
        else:
            idx = self.shard(idx, rank, world)                   # data parallelism: equal-length strided shards of the epoch
        # (start_batch > 0: the first batches of the epoch are skipped - no augmentation draw, no launch)
        for b0 in range(start_batch * self.batch_size, len(idx), self.batch_size):
            yield self.make_batch([self.draw_sample(i, train, gen) for i in idx[b0:b0 + self.batch_size]])

    def train_dataloader(self, rank=0, world=1, start_batch=0):
        """start_batch: begin at that batch of the epoch (a resumed run, after load_state_dict: the epoch's order is re-drawn from the
        saved epoch-start state of the shuffle generator, which ends up where the uninterrupted run's is)."""
        return self._loader(self.train_idx, True, True, rank, world, "train", start_batch)

    def state_dict(self):
        """The shuffle generator's state at the start of the current training epoch (before the first epoch: its current state) and the
        current state of every augmentation generator of this rank (train and eval; they draw lazily, batch by batch).  The position
        inside the epoch is the trainer's `batches_into_epoch`."""
        st = self._gen.get_state() if self._epoch_gen_state is None else self._epoch_gen_state
        sd = {"kind": type(self).__name__, "seed": self._seed, "nsamples": int(self.nsamples), "batch_size": int(self.batch_size),
              "crop": int(self.crop), "stage": self.stage, "epoch_gen_state": st.clone(),
              "aug_generators": {f"{k}:{r}": g.get_state() for (k, r), g in self._aug_gens.items()}}
        if any(self._norm_from_file):                            # constants of a file ($VDM4CDM_NORMALIZATIONS): a resume must find the same
            sd["norm"] = self._norm_state()
        return sd

    def _norm_state(self):
        return [[float(a), float(m), float(s)] for a, m, s in zip(self.alphas, self.means, self.stds)]

    def load_state_dict(self, state):
        mine = self.state_dict()
        if isinstance(state, dict) and "norm" in state:          # compared whenever the saved run recorded them; a state without the
            mine["norm"] = self._norm_state()                    # key (every default run) is accepted as it always was
        else:
            mine.pop("norm", None)
        _check_same_module(mine, state, skip=("epoch_gen_state", "aug_generators"))
        self._gen.set_state(state["epoch_gen_state"])
        self._epoch_gen_state = state["epoch_gen_state"].clone()
        for key, st in state["aug_generators"].items():
            kind, rank = key.rsplit(":", 1)
            self._aug_generator(kind, int(rank)).set_state(st)

    def val_dataloader(self, rank=0, world=1):
        return self._loader(self.valid_idx, True, False, rank, world, "eval")          # (the reference's valid split shares the "fit" transforms)

    def test_dataloader(self, rank=0, world=1):
        return self._loader(self.test_idx, False, False, rank, world, "eval")


def _check_same_module(mine, saved, skip=()):
    """ValueError unless the saved data-module state was written by a module configured like this one."""
    if not isinstance(saved, dict) or saved.get("kind") != mine["kind"]:
        raise ValueError(f"data-module state of a {saved.get('kind') if isinstance(saved, dict) else type(saved).__name__} cannot be loaded "
                         f"into a {mine['kind']}")
    bad = [f"{k}: saved {saved.get(k)!r}, this module {v!r}" for k, v in mine.items() if k not in skip and saved.get(k) != v]
    if bad:
        raise ValueError(f"the data-module state does not match this {mine['kind']} ({'; '.join(bad)}): a run resumes only on the data "
                         "module configuration that it was started with")


def _cv_keep(n):
    """CV set: simulations 2, 8 and 17 are excluded (/root/reference/src/dataset/CAMELS_3D_dataset.py:112-117)."""
    keep = np.ones(n, dtype=bool)
    keep[[i for i in (2, 8, 17) if i < n]] = False
    return keep


def write_synthetic_camels(root, dataset_name="CMD_128", suite_name="Astrid", set_name="LH", z_name="z_0.0",
                           channel_names=("Mstar", "Mcdm"), n_sims=4, fullsize=None, seed=0):
    """Writes a small synthetic data set in the reference's on-disk layout (raw, un-normalised densities + the parameter table),
    so that the file-backed module and the entry scripts can be exercised without the CAMELS files.  `fullsize` overrides the grid
    size the dataset name implies (tests)."""
    S = fullsize or grid_size(dataset_name)
    g = torch.Generator().manual_seed(seed)
    x = gaussian_random_field((n_sims, 1, S, S, S), generator=g)[:, 0]
    for c in channel_names:
        m, s = NORMALIZATIONS[c]
        if c == "Mstar":
            rho = torch.relu(10 ** (1.2 * (x - 1.0)) - 1.0)           # sparse, with exact zeros
        else:
            rho = 10 ** (x * s + m) - ALPHAS[c]
        p = field_path(root, dataset_name, suite_name, set_name, z_name, c)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        np.save(p, rho.clamp(min=0).numpy().astype(np.float32))
    params = (PARAM_LO + (PARAM_HI - PARAM_LO) * torch.rand(n_sims, 6, generator=g)).numpy()
    os.makedirs(os.path.dirname(params_path(root, suite_name, set_name)), exist_ok=True)
    np.savetxt(params_path(root, suite_name, set_name), params)
    return root


def make_down_grids(root, nside, fields=("Mcdm", "Mstar"), sets=("LH", "CV", "1P"), suite="Astrid", z="z_0.0", overwrite=False,
                    device=None, verbose=True):
    """The reference's data-preparation step (scripts/make_down_grids.ipynb) on the device: every 256^3 stack
    3D_grids_new/Grids_<field>_<suite>_<set>_256_z=....npy below `root` becomes the float32 stack (n, T, T, T) of data set
    CMD_<nside> at ``field_path(root, f"CMD_{nside}", ...)``, T = nside * (edge found in the source) / 256, resampled by
    ``vdm_downgrid_trilinear`` (F.interpolate(mode="trilinear", align_corners=False) semantics).  The defaults are the six stacks the
    notebook converts; the parameter tables are shared between the sizes, so nothing else is written.

    Every source is checked first - a missing one, an `nside` outside 1..256 or a non-integer T raises ValueError before any GPU
    work.  A stack is uploaded in slabs of whole simulations (<= 1 GiB), resampled, and copied back into a temporary file of the target
    directory that replaces the final name only when complete: an interrupted run never leaves a truncated .npy.  An existing target is
    kept unless `overwrite`.  Returns one record per stack: {"path", "status" ("written" | "kept"), "shape", "seconds": {"read", "h2d",
    "kernel", "d2h", "write"}} (the phases are separated by device synchronisations: this is a tool, not the training path)."""
    import time
    if not root:
        raise ValueError(f"make_down_grids needs the CAMELS directory (root= or ${DATA_ROOT_ENV})")
    down_grid_edge(nside, 256)                              # (the range of nside, whatever the sources hold)
    plan = []
    for c in fields:
        for set_name in sets:
            src = field_path(root, "CMD", suite, set_name, z, c)
            if not os.path.exists(src):
                raise ValueError(f"make_down_grids: the 256^3 source stack {src} does not exist")
            f = np.load(src, mmap_mode="r")
            if f.ndim != 4 or f.shape[1:] != (f.shape[-1],) * 3:
                raise ValueError(f"make_down_grids: {src} has shape {f.shape}, not a stack of cubes (n, S, S, S)")
            plan.append((src, f, down_grid_edge(nside, f.shape[-1]), field_path(root, f"CMD_{nside}", suite, set_name, z, c)))
    dev = torch.device(device if device is not None else "cuda")
    report = []
    for src, f, T, dst in plan:
        shape = (len(f), T, T, T)
        if os.path.exists(dst) and not overwrite:
            report.append({"path": dst, "status": "kept", "shape": shape, "seconds": {}})
            if verbose:
                print(f"[make_down_grids] {dst} exists: kept (--overwrite rewrites it)", flush=True)
            continue
        from . import hip_ops as ops
        sec = dict.fromkeys(("read", "h2d", "kernel", "d2h", "write"), 0.0)

        def lap(key, t0):
            torch.cuda.synchronize(dev)
            sec[key] += time.perf_counter() - t0
            return time.perf_counter()

        os.makedirs(os.path.dirname(dst), exist_ok=True)
        tmp = os.path.join(os.path.dirname(dst), f".{os.path.basename(dst)}.tmp{os.getpid()}")
        try:
            out = np.lib.format.open_memmap(tmp, mode="w+", dtype=np.float32, shape=shape)
            step = _slab_sims(f)
            slab = torch.empty((min(step, len(f)),) + tuple(f.shape[1:]), dtype=torch.float32, device=dev)
            small = torch.empty((slab.shape[0], T, T, T), dtype=torch.float32, device=dev)
            with torch.cuda.device(dev):
                for i in range(0, len(f), step):
                    k = min(step, len(f) - i)
                    t0 = time.perf_counter()
                    host = torch.from_numpy(np.array(f[i:i + k], dtype=np.float32))      # (a copy: the read happens here, not in the upload)
                    t0 = lap("read", t0)
                    slab[:k].copy_(host)
                    t0 = lap("h2d", t0)
                    ops.downgrid_trilinear(slab[:k], T, out=small[:k])
                    t0 = lap("kernel", t0)
                    back = small[:k].cpu().numpy()
                    t0 = lap("d2h", t0)
                    out[i:i + k] = back
                    lap("write", t0)
            t0 = time.perf_counter()
            out.flush()
            del out
            os.replace(tmp, dst)
            sec["write"] += time.perf_counter() - t0
        finally:
            if os.path.exists(tmp):
                os.remove(tmp)
        report.append({"path": dst, "status": "written", "shape": shape, "seconds": sec})
        if verbose:
            print(f"[make_down_grids] {src} -> {dst} {shape}: " + ", ".join(f"{k} {v:.2f} s" for k, v in sec.items()), flush=True)
    return report


def merge_log_moments(records, pivot):
    """(n, mean, std, min, max, n_bad) of log10(field + alpha) from the per-slab records of ``hip_ops.log_moments`` taken with ONE
    `pivot`: the shifted sums add (math.fsum: exactly rounded), mean = pivot + S1/N, std = sqrt(max(S2/N - (S1/N)^2, 0)) - the
    population std (ddof = 0) that np.std gives in the reference's notebook.  Pure Python float64.  Without a valid element mean and
    std are NaN."""
    records = list(records)
    n = sum(int(r["n_valid"]) for r in records)
    n_bad = sum(int(r["n_bad"]) for r in records)
    lo = min([float(r["min"]) for r in records], default=math.inf)
    hi = max([float(r["max"]) for r in records], default=-math.inf)
    if n == 0:
        return 0, math.nan, math.nan, lo, hi, n_bad
    m1 = math.fsum(float(r["S1"]) for r in records) / n
    m2 = math.fsum(float(r["S2"]) for r in records) / n
    return n, float(pivot) + m1, math.sqrt(max(m2 - m1 * m1, 0.0)), lo, hi, n_bad


def _normalization_source(root, field, suite, set_name, z, nside, alpha):
    """(path, memory-mapped stack, alpha) of one field_normalization call, or ValueError - everything that can be refused without a GPU."""
    if not root:
        raise ValueError(f"field_normalization needs the CAMELS directory (root= or ${DATA_ROOT_ENV})")
    if alpha is None:
        if field not in ALPHAS:
            raise ValueError(f"field_normalization: no alpha of log10(field + alpha) is known for field {field!r} (known: "
                             f"{sorted(ALPHAS)}): give one (alpha= / --alpha)")
        alpha = ALPHAS[field]
    alpha = float(alpha)
    if not math.isfinite(alpha):
        raise ValueError(f"field_normalization: alpha = {alpha!r} is not finite")
    if isinstance(nside, bool) or not isinstance(nside, (int, np.integer)) or nside < 1:
        raise ValueError(f"field_normalization: nside = {nside!r} must be a positive integer")
    path = field_path(root, "CMD" if nside == 256 else f"CMD_{nside}", suite, set_name, z, field)
    if not os.path.exists(path):
        raise ValueError(f"field_normalization: the stack {path} does not exist")
    f = np.load(path, mmap_mode="r")
    if f.ndim != 4 or f.shape[1:] != (f.shape[-1],) * 3 or f.size == 0:
        raise ValueError(f"field_normalization: {path} has shape {f.shape}, not a stack of cubes (n, S, S, S)")
    return path, f, alpha


def field_normalization(root, field, suite="Astrid", set_name="LH", z="z_0.0", nside=256, alpha=None, slab_sims=None, device=None):
    """The normalisation constants of one field - mean and population std of log10(field + alpha) in float64 over the whole stack
    ``field_path(root, ...)`` - as the reference's scripts/calc_normalization.ipynb computes them on the host
    (np.log10(stack.astype(np.float64) + alpha), .mean(), .std()), in one streaming pass on the device: the memory-mapped stack is
    uploaded in slabs of whole simulations (`slab_sims`, default at most 1 GiB as in the training module), every slab is one
    ``vdm_log_moments`` call with the same pivot (log10(first element + alpha)), and the records are merged once
    (``merge_log_moments``).  `alpha` defaults to ALPHAS[field].

    ValueError before any GPU work: no root, a missing stack, a stack that is not (n, S, S, S), no alpha for the field.  ValueError
    after the pass: elements that are not finite or have field + alpha <= 0 (the reference's constants would be NaN there), or std == 0.
    Returns {"field", "path", "mean", "std", "alpha", "n", "min", "max", "pivot", "seconds": {"read", "h2d", "kernel"}}."""
    import time
    path, f, alpha = _normalization_source(root, field, suite, set_name, z, nside, alpha)
    step = _slab_sims(f) if slab_sims is None else int(slab_sims)
    if step < 1:
        raise ValueError(f"field_normalization: slab_sims = {slab_sims!r} must be at least 1")
    first = float(np.float32(f[0, 0, 0, 0])) + alpha
    pivot = math.log10(first) if math.isfinite(first) and first > 0 else 0.0
    dev = torch.device(device if device is not None else "cuda")
    if dev.type != "cuda":
        raise RuntimeError("field_normalization runs a HIP kernel: device must be a GPU (there is no CPU path)")
    from . import hip_ops as ops
    sec = dict.fromkeys(("read", "h2d", "kernel"), 0.0)

    def lap(key, t0):
        torch.cuda.synchronize(dev)
        sec[key] += time.perf_counter() - t0
        return time.perf_counter()

    records, worst = [], math.inf
    with torch.cuda.device(dev):
        slab = torch.empty((min(step, len(f)),) + tuple(f.shape[1:]), dtype=torch.float32, device=dev)
        for i in range(0, len(f), step):
            k = min(step, len(f) - i)
            t0 = time.perf_counter()
            host = np.array(f[i:i + k], dtype=np.float32)             # (a copy: the read happens here, not in the upload)
            t0 = lap("read", t0)
            slab[:k].copy_(torch.from_numpy(host))
            t0 = lap("h2d", t0)
            records.append(ops.log_moments(slab[:k], alpha, pivot))
            lap("kernel", t0)
            if records[-1]["n_bad"]:
                worst = min(worst, float(np.nanmin(host)) if not np.isnan(host).all() else math.nan)
    n, mean, std, lo, hi, n_bad = merge_log_moments(records, pivot)
    if n_bad:
        raise ValueError(f"field_normalization: {n_bad} of {n + n_bad} elements of {path} are not finite or have field + alpha <= 0 "
                         f"(smallest value seen {worst!r}, alpha = {alpha!r}): log10(field + alpha) is undefined there and the reference's "
                         "constants would be NaN - clean the stack or give a larger alpha")
    if not std > 0:
        raise ValueError(f"field_normalization: log10({field} + {alpha!r}) is constant over {path} (std == 0, mean {mean!r}): it cannot "
                         "be normalised")
    return {"field": field, "path": path, "mean": mean, "std": std, "alpha": alpha, "n": n, "min": lo, "max": hi, "pivot": pivot,
            "seconds": sec}


def calc_normalizations(root, fields, suite="Astrid", set_name="LH", z="z_0.0", nside=256, alpha=None, out="normalizations_3d.json",
                        device=None, verbose=True):
    """``field_normalization`` for every field of `fields`, merged into the JSON file `out` in the reference's flat schema
    {"<field>_m": mean, "<field>_s": std} (full float64 repr): entries of other fields are kept, the named fields are replaced.  The
    file is rewritten after every field through a temporary file and os.replace, so an interrupted or failing run leaves the last
    complete file.  Every source and the existing `out` are checked before any GPU work.  Returns the list of field records; a field
    with built-in constants also reports how far the new ones are from them ("builtin", printed, never asserted)."""
    import json
    fields = list(fields)
    if not fields:
        raise ValueError("calc_normalizations: no field given")
    for c in fields:
        _normalization_source(root, c, suite, set_name, z, nside, alpha)
    if os.path.exists(out):
        load_normalizations(out)                                # (a file this tool could not have written is not overwritten)
    report = []
    for c in fields:
        rec = field_normalization(root, c, suite=suite, set_name=set_name, z=z, nside=nside, alpha=alpha, device=device)
        merged = {}
        if os.path.exists(out):
            with open(out) as fh:
                merged = json.load(fh)
        merged[f"{c}_m"], merged[f"{c}_s"] = rec["mean"], rec["std"]
        tmp = os.path.join(os.path.dirname(os.path.abspath(out)), f".{os.path.basename(out)}.tmp{os.getpid()}")
        try:
            with open(tmp, "w") as fh:
                json.dump(merged, fh, indent=2)
                fh.write("\n")
            os.replace(tmp, out)
        finally:
            if os.path.exists(tmp):
                os.remove(tmp)
        line = (f"[calc_normalization] {c}: mean = {rec['mean']!r}, std = {rec['std']!r} (alpha {rec['alpha']:g}, n = {rec['n']}, min "
                f"{rec['min']:g}, max {rec['max']:g}; " + ", ".join(f"{k} {v:.2f} s" for k, v in rec["seconds"].items()) + f") -> {out}")
        if c in NORMALIZATIONS:
            m0, s0 = NORMALIZATIONS[c]
            rec["builtin"] = {"mean": m0, "std": s0, "d_mean": rec["mean"] - m0, "d_std": rec["std"] - s0}
            line += f"; built-in ({m0!r}, {s0!r}): mean {rec['mean'] - m0:+.3e}, std {rec['std'] - s0:+.3e}"
        if verbose:
            print(line, flush=True)
        report.append(rec)
    return report


def get_dataset(dataset_name="CMD_128", suite_name="Astrid", return_func=None, set_name="LH", z_name="z_0.0",
                channel_names=("Mstar", "Mcdm"), stage="fit", batch_size=2, cropsize=128, ndim=3, num_workers=0, mmap=False,
                data_root=None, **kw):
    """Signature of the reference's ``CAMELS_3D_dataset.get_dataset`` (/root/reference/src/dataset/CAMELS_3D_dataset.py:202-234).
    With the CAMELS directory given (``data_root=`` or $VDM4CDM_DATA_ROOT, files laid out as on the reference's cluster) this is the
    file-backed ``AstroDataModule``; otherwise - LOUDLY - the seeded synthetic module with the same batch contract."""
    root = data_root or os.environ.get(DATA_ROOT_ENV)
    if root:
        selection = {"dataset_name": dataset_name, "suite_name": suite_name, "set_name": set_name, "z_name": z_name}
        return AstroDataModule(selection=selection, channel_names=list(channel_names), return_func=return_func, stage=stage,
                               batch_size=batch_size, do_crop=cropsize != 256, cropsize=cropsize, ndim=ndim,
                               num_workers=num_workers, mmap=mmap, data_root=root, **kw)
    warnings.warn(f"${DATA_ROOT_ENV} is not set: {dataset_name}/{suite_name}/{set_name} is replaced by SYNTHETIC lognormal fields "
                  "(same batch contract, not CAMELS data)", stacklevel=2)
    n = {"LH": 1000, "CV": 27, "1P": 61}.get(set_name, 1000)
    if stage == "fit":
        n_train, n_val, n_test = int(0.95 * n), n - int(0.95 * n), 0
    else:
        n_train, n_val, n_test = 0, 0, max(n - 3, 1)          # CV sims 2/8/17 are excluded upstream
    return SyntheticAstroDataModule(cropsize=cropsize, batch_size=batch_size, dim=3, n_train=max(n_train, batch_size),
                                    n_val=max(n_val, batch_size), n_test=max(n_test, 1), channel_names=channel_names,
                                    return_func=return_func, **kw)
