"""detzero_track.utils.data_utils (tracking/detzero_track/utils/data_utils.py:8-76): the frame / sequence containers."""
from detzero_amd.track_adapter import (dict_to_sequence_list, frame_list_to_dict, sequence_list_to_dict,  # noqa: F401
                                       tracklets_to_frames)
