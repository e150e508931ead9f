"""torch.hub entry points with the reference's signatures (its hubconf.py):

    ddpm, lidar_utils, cfg = torch.hub.load("<this repo>", "pretrained_r2dm", device="cuda")
    x = ddpm.sample(batch_size=8, num_steps=256)          # MI355X HIP kernels, see r2dm_amd/

and the reference's RangeNet++ entries (hubconf.py:45-104), also as HIP kernels (r2dm_amd.rangenet, r2dm_amd.postproc):

    model, preprocess = torch.hub.load("<this repo>", "rangenet", "/data/darknet53-1024.tar.gz")
    logits = model(preprocess(img, mask))                 # (B,20,H,W); model(x, feature="lidargen") is the FRD feature
    knn = torch.hub.load("<this repo>", "knn")            # kNN label filter of RangeNet++
    crf = torch.hub.load("<this repo>", "crf_rnn")        # CRF-RNN refinement of SqueezeSeg

A local path never touches the network; a URL, and the weight names of ``rangenet21`` / ``rangenet53``, go through torch.hub's
checkpoint cache, as ``pretrained_r2dm`` does."""
dependencies = ["torch", "numpy"]


def _get_r2dm_url(key: str) -> str:
    return f"https://github.com/kazuto1011/r2dm/releases/download/weights/{key}.pth"


def pretrained_r2dm(config: str = "r2dm-h-kitti360-300k", ckpt: str = None, **kwargs):
    """R2DM sampler from a released checkpoint.

    Args:
        config: release key of the pre-trained weights (default "r2dm-h-kitti360-300k").
        ckpt:   path to (or dict of) a checkpoint; if given, `config` is ignored.
        **kwargs: forwarded to ``r2dm_amd.setup_model`` (device=..., ema=..., show_info=..., max_batch=...).
    Returns:
        (ddpm, lidar_utils, cfg) exactly like the reference.
    """
    from r2dm_amd import setup_model

    if ckpt is None:
        from torch.hub import load_state_dict_from_url

        ckpt = load_state_dict_from_url(_get_r2dm_url(config), map_location="cpu")
    return setup_model(ckpt, **kwargs)


def _named_rangenet(backbone: int, weights: str, **kwargs):
    from r2dm_amd import rangenet as rn

    if weights is None:
        raise ValueError(f"rangenet{backbone}: weights=None would be an untrained network; name the weights or use rangenet(url_or_file)")
    if weights not in rn.OFFICIAL_ARCHIVES[backbone]:
        raise ValueError(f"rangenet{backbone}: weights must be one of {sorted(rn.OFFICIAL_ARCHIVES[backbone])}, got {weights!r}")
    return rn.build_rangenet(rn.official_url(rn.OFFICIAL_ARCHIVES[backbone][weights]), **kwargs)


def rangenet(url_or_file: str, **kwargs):
    """RangeNet-21 / -53 from a checkpoint archive (*.tar.gz): a local path or a URL.  ``**kwargs``: ``device`` (default "cuda").

    Returns:
        (model, preprocess): ``model(preprocess(img, mask), feature=None)``.
    """
    from r2dm_amd import rangenet as rn

    return rn.build_rangenet(url_or_file, **kwargs)


def rangenet21(weights: str = "SemanticKITTI_64x2048", **kwargs):
    """RangeNet-21 pre-trained on SemanticKITTI: weights "SemanticKITTI_64x2048".  Returns (model, preprocess)."""
    return _named_rangenet(21, weights, **kwargs)


def rangenet53(weights: str = "SemanticKITTI_64x2048", **kwargs):
    """RangeNet-53 pre-trained on SemanticKITTI: weights "SemanticKITTI_64x2048", "SemanticKITTI_64x1024" or "SemanticKITTI_64x512".
    Returns (model, preprocess)."""
    return _named_rangenet(53, weights, **kwargs)


def knn(num_classes: int = 20, **kwargs):
    """kNN post-processing of RangeNet++ (``r2dm_amd.postproc.KNN``): ``knn(depth, label) -> label``."""
    from r2dm_amd.postproc import KNN

    return KNN(num_classes, **kwargs)


def crf_rnn(num_classes: int = 20, **kwargs):
    """CRF-RNN post-processing (``r2dm_amd.postproc.CRFRNN``): ``crf(unary, xyz, mask) -> Q``."""
    from r2dm_amd.postproc import CRFRNN

    return CRFRNN(num_classes, **kwargs)
