"""Videos that live in a single file (the reference's `video/io/file.py`).

The reference chooses between an ffmpeg and an OpenCV backend; here the one backend is Motion-JPEG in an AVI
container, encoded on the GPU (`backend_mjpeg.py`).  `write_video` and `load_any_video` keep the reference's
signatures (file.py:37-64); videos spread over several files (`VideoFileStack`, patterns with `*`, `?` or `%`) are
not supported.
"""
import logging
import os

from .backend_mjpeg import VideoMJPEG, VideoWriterMJPEG

logger = logging.getLogger("video.io")

VideoFile = VideoMJPEG
VideoFileWriter = VideoWriterMJPEG


def load_any_video(video_filename_pattern, parameters=None):
    """loads a video file; a pattern that names a stack of files raises NotImplementedError"""
    if any(c in os.fspath(video_filename_pattern) for c in r"*?%"):
        raise NotImplementedError("video file stacks (a pattern with * ? or %%) are not supported: %r"
                                  % (video_filename_pattern,))
    return VideoFile(video_filename_pattern, parameters=parameters)


def write_video(video, filename, **kwargs):
    """Saves the video to the file indicated by filename.  The extra arguments go to the video writer
    (`quality`, `batch`)."""
    with VideoFileWriter(filename, size=video.size, fps=video.fps, is_color=video.is_color, **kwargs) as writer:
        for frame in video:
            writer.write_frame(frame)
