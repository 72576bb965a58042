"""Train-time augmentation on the device (reference: datasets/data_transforms.py): the reference's seven transforms and a Compose.

PointcloudScaleAndTranslate: per sample, per axis scale ~ U[2/3, 3/2] and shift ~ U[-0.2, 0.2], applied in place
by one HIP launch (act_scale_translate_f32) with draws sampled on the device: no Python loop over the batch and
no per-sample host->device copies (the reference does 2 numpy draws + 2 tiny H2D copies per sample).
PointcloudRotate likewise (act_rotate_points_f32).  The other five classes and Compose, further down, go through act_augment_f32: a chain of
up to 8 ops in one launch, the cloud held in LDS, the draws from Philox inside the kernel."""
import torch

from .. import _C


class PointcloudScaleAndTranslate(object):
    def __init__(self, scale_low=2. / 3., scale_high=3. / 2., translate_range=0.2):
        self.scale_low = scale_low
        self.scale_high = scale_high
        self.translate_range = translate_range

    def __call__(self, pc, scale=None, shift=None):
        """pc f32 [B,N,3] CUDA, modified in place and returned.  ``scale``/``shift`` [B,3] inject the draws."""
        B, N, C = pc.shape
        if C != 3 or not pc.is_cuda:
            raise RuntimeError("PointcloudScaleAndTranslate expects a CUDA tensor [B, N, 3]")
        if scale is None:
            scale = torch.empty(B, 3, device=pc.device).uniform_(self.scale_low, self.scale_high)
        if shift is None:
            shift = torch.empty(B, 3, device=pc.device).uniform_(-self.translate_range, self.translate_range)
        scale = scale.to(pc.device, torch.float32).contiguous(); shift = shift.to(pc.device, torch.float32).contiguous()
        _C.check(_C.lib.act_scale_translate_f32(_C.ptr(pc), _C.ptr(scale), _C.ptr(shift), B, N, _C.stream()),
                 "act_scale_translate_f32")
        return pc


class PointcloudRotate(object):
    """Random rotation about the y axis per sample (datasets/data_transforms.py:6-18): pc[i] @ [[c,0,s],[0,1,0],[-s,0,c]],
    angle = 2*pi*U[0,1).  One HIP launch (act_rotate_points_f32); the angles are drawn on the device."""

    def __call__(self, pc, u=None):
        """pc f32 [B,N,3] CUDA, modified in place and returned.  ``u`` [B] in [0,1) injects the draws."""
        B, N, C = pc.shape
        assert C == 3 and pc.is_contiguous() and pc.dtype == torch.float32
        if u is None:
            u = torch.rand(B, device=pc.device, dtype=torch.float64)
        ang = torch.as_tensor(u, dtype=torch.float64, device=pc.device) * (2 * torch.pi)
        c, s = torch.cos(ang), torch.sin(ang)
        z, o = torch.zeros_like(c), torch.ones_like(c)
        rot = torch.stack((c, z, s, z, o, z, -s, z, c), dim=1).to(torch.float32).contiguous()      # [B,9]
        _C.check(_C.lib.act_rotate_points_f32(_C.ptr(pc), _C.ptr(rot), B, N, _C.stream()), "act_rotate_points_f32")
        return pc


# ---- the remaining five transforms and Compose: chains of ops of ONE launch (act_augment_f32, csrc/augment.hip) ---------------------------------
# Every class below is a one-op chain; Compose runs any chain of the seven classes as one launch, the cloud held in LDS between the ops and the
# draws taken from Philox inside the kernel (or injected by keyword, as the two classes above do).  Each class names its op through
# ``_op()`` -> (kind, p0, p1, p2) and its injectable draws through ``_draw_names``.
def _host_seed():
    return int(torch.randint(0, 2 ** 62, (1,)).item())          # torch's generator on the host: no device sync


def _run_chain(pc, ops, draws, seed):
    from .. import kernels as K
    if pc.dim() != 3 or pc.shape[2] != 3 or not pc.is_cuda:
        raise RuntimeError("point-cloud transforms expect a CUDA tensor [B, N, 3]")
    return K.augment(pc, ops, draws, _host_seed() if seed is None else seed)


class _ChainOp(object):
    _draw_names = ()

    def __call__(self, pc, *args, seed=None, **kw):
        """pc f32 [B,N,3] CUDA, modified in place and returned; the draws can be injected by keyword (or position), else Philox keyed by ``seed``
        (None: a seed from torch's generator)."""
        given = dict(zip(self._draw_names, args))
        for k, v in kw.items():
            if k not in self._draw_names or k in given:
                raise TypeError(f"{type(self).__name__}: unexpected draw {k!r} (takes {self._draw_names})")
            given[k] = v
        return _run_chain(pc, [self._op()], [tuple(given.get(n) for n in self._draw_names)], seed)


class PointcloudJitter(_ChainOp):
    """p += clamp(N(0, std), -clip, clip) per point and axis (datasets/data_transforms.py:36-48).  ``noise`` [B,N,3] injects the N(0,1) draws."""
    _draw_names = ("noise",)

    def __init__(self, std=0.01, clip=0.05):
        self.std, self.clip = std, clip

    def _op(self):
        from .. import kernels as K
        return (K.AUG_JITTER, self.std, self.clip, 0.)


class PointcloudScale(_ChainOp):
    """per sample, per axis scale ~ U[scale_low, scale_high) (datasets/data_transforms.py:50-62).  ``scale`` [B,3] injects the draws."""
    _draw_names = ("scale",)

    def __init__(self, scale_low=2. / 3., scale_high=3. / 2.):
        self.scale_low = scale_low
        self.scale_high = scale_high

    def _op(self):
        from .. import kernels as K
        return (K.AUG_SCALE, self.scale_low, self.scale_high, 0.)


class PointcloudTranslate(_ChainOp):
    """per sample, per axis shift ~ U[-translate_range, translate_range) (datasets/data_transforms.py:64-75).  ``shift`` [B,3] injects the draws."""
    _draw_names = ("shift",)

    def __init__(self, translate_range=0.2):
        self.translate_range = translate_range

    def _op(self):
        from .. import kernels as K
        return (K.AUG_TRANSLATE, self.translate_range, 0., 0.)


class PointcloudRandomInputDropout(_ChainOp):
    """per sample ratio = U[0,1) * max_dropout_ratio; every point whose own uniform is <= ratio becomes a copy of point 0
    (datasets/data_transforms.py:78-93).  ``ratio`` [B] and ``drop_u`` [B,N] inject the two sets of uniforms."""
    _draw_names = ("ratio", "drop_u")

    def __init__(self, max_dropout_ratio=0.5):
        assert max_dropout_ratio >= 0 and max_dropout_ratio < 1
        self.max_dropout_ratio = max_dropout_ratio

    def _op(self):
        from .. import kernels as K
        return (K.AUG_DROPOUT, self.max_dropout_ratio, 0., 0.)


class RandomHorizontalFlip(_ChainOp):
    """with probability 0.95, each horizontal axis is mirrored with probability 0.5: x = max_n(x) - x (datasets/data_transforms.py:95-117).
    ``flip_u`` [B,3] injects (gate, first horizontal axis, second), the horizontal axes in ascending order.  4-D temporal coordinates are not
    supported."""
    _draw_names = ("flip_u",)

    def __init__(self, upright_axis='z', is_temporal=False):
        if is_temporal:
            raise ValueError("RandomHorizontalFlip(is_temporal=True) is not supported: clouds are [B, N, 3]")
        self.upright_axis = "xyz".index(upright_axis.lower())          # the kernel mirrors the other two axes

    def _op(self):
        from .. import kernels as K
        return (K.AUG_FLIP, float(self.upright_axis), 0., 0.)


def _chain_entry(t):
    """(op, draw names) of a member of a Compose; the two single-launch classes become SCALE_TRANSLATE / ROTATE_Y ops"""
    from .. import kernels as K
    if isinstance(t, _ChainOp):
        return t._op(), t._draw_names
    if isinstance(t, PointcloudScaleAndTranslate):
        return (K.AUG_SCALE_TRANSLATE, t.scale_low, t.scale_high, t.translate_range), ("scale", "shift")
    if isinstance(t, PointcloudRotate):
        return (K.AUG_ROTATE_Y, 0., 0., 0.), ("u",)
    raise TypeError(f"Compose takes the transforms of this module ({', '.join(TRANSFORM_NAMES)}), got {type(t).__name__}")


TRANSFORM_NAMES = ("PointcloudRotate", "PointcloudScaleAndTranslate", "PointcloudJitter", "PointcloudScale", "PointcloudTranslate",
                   "PointcloudRandomInputDropout", "RandomHorizontalFlip")


class Compose(object):
    """A chain of up to 8 of the seven transforms, applied in order by ONE launch.  ``draws``: {"{position}.{name}": tensor} with the names
    scale, shift, u, noise, ratio, drop_u, flip_u; ``seed``: the Philox seed of the draws that are not injected (None: from torch's generator)."""

    def __init__(self, transforms):
        self.transforms = list(transforms)
        for t in self.transforms:
            _chain_entry(t)                                     # TypeError at construction
        if not 1 <= len(self.transforms) <= 8:
            raise ValueError(f"Compose takes 1 to 8 transforms, got {len(self.transforms)}")

    def __call__(self, pc, draws=None, seed=None):
        entries = [_chain_entry(t) for t in self.transforms]    # (read at call time: a member's parameters may be changed after construction)
        draws = dict(draws or {})
        inj = [tuple(draws.pop(f"{i}.{n}", None) for n in names) for i, (_, names) in enumerate(entries)]
        if draws:
            raise KeyError(f"Compose: no such draws {sorted(draws)}")
        return _run_chain(pc, [op for op, _ in entries], inj, seed)


def build_transforms(spec):
    """Compose from the YAML key ``train_transforms``: a list of {NAME: <class>, <keyword arguments>}"""
    members = []
    for item in spec:
        kw = dict(item)
        name = kw.pop("NAME", None)
        if name not in TRANSFORM_NAMES:
            raise ValueError(f"train_transforms: unknown transform {name!r}; the transforms are {', '.join(TRANSFORM_NAMES)}")
        members.append(globals()[name](**kw))
    return Compose(members)
