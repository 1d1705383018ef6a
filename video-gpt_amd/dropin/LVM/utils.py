from video_gpt_amd.vae import vae_encode, vae_encode_list  # noqa: F401
from video_gpt_amd.sequence_parallel import broadcast_batch  # noqa: F401


def broadcast_data(data, src, group, device=None):
    """LVM/utils.py: the scripts' name and argument order for sequence_parallel.broadcast_batch."""
    return broadcast_batch(data, src, group, device)
