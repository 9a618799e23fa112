"""The trained system of a command-line tool (extract_mesh.py, render_path.py)."""


def load_system(config=None, ckpt=None, need_dataset=False):
    """NeRFSystem of the scene's YAML `config` (its dataset loaded) holding the checkpoint `ckpt`, on the GPU.  Without `config`
    the hyper-parameters come from the checkpoint and the dataset is a poseless SyntheticDataset: need_dataset refuses that."""
    from upnerf_amd import checkpoint, config as cfg
    from upnerf_amd.nerf_system import NeRFSystem, SyntheticDataset
    state = checkpoint.read_checkpoint(ckpt) if ckpt else None
    if config:
        system = NeRFSystem(cfg.get_from_path(config))
    else:
        if "hyper_parameters" not in state:
            raise SystemExit("the checkpoint carries no hyper-parameters: give --config")
        if need_dataset:
            raise SystemExit("--from-cameras needs the dataset's poses: give --config, or --bounds")
        sd = state.get("state_dict", state)
        system = NeRFSystem(dict(state["hyper_parameters"]), SyntheticDataset(sd["se3_refine.weight"].shape[0]))
    system.setup()
    if state is not None:
        checkpoint.load_checkpoint(system, state, resume=False)
    return system.cuda()
