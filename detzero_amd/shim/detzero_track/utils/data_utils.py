"""detzero_track.utils.data_utils (tracking/detzero_track/utils/data_utils.py:8-30): the frame / sequence containers."""
from detzero_amd.track_adapter import dict_to_sequence_list, frame_list_to_dict, sequence_list_to_dict  # noqa: F401
