"""Module2 side of the end-to-end driver, in one process -- counterpart of ``test_gan_new`` and the frame / video steps of
main_end2end_module2.py:90-124, 294-343.

The reference writes one landmark txt + one landmark PNG per frame, shells out to ``python test.py --model
geomcgt_ifw_test`` (which re-reads them, builds the motion grids with scipy on the CPU and runs the model at batch 1),
copies the PNGs it wrote and calls ffmpeg at 62.5 fps.  Here: photo + a landmark clip in, frames (and the video, when
ffmpeg exists) out, through ``stream.ClipStreamer`` in batches.  ``--video avi`` needs no ffmpeg: the frames are encoded as
JPEG on the GPU and muxed with the sound into ``<out>/output.avi`` here (util/avi.py); ``--frames none`` then skips the PNGs.
``--landmark_video avi`` adds ``<out>/landmark_seq2.avi``, the driving landmarks as coloured face contours (:47-68, 303), and
``--side_outputs`` adds ``photo.png`` and ``ori_view.png`` (:286, 328-331): what the generator was given, drawn on the GPU.

    python -m animateportrait_amd.end2end --photo face.png --landmarks Data/Alm_txt/MTCNN/<db>_MTCNN \\
        --landmark_scale 0.5 --name formal/drawing --epoch 70 --out output/<db> [--audio a.wav]

Landmark sources: ``--landmarks DIR`` (the reference's ``Alm_txt`` layout: ``ori.txt`` + ``%05d.txt``, 512-px coordinates
for a 256-px photo -> ``--landmark_scale 0.5``), ``--landmarks_npy FILE`` ((T + 1, 68, 2): row 0 = the photo's), or the audio
itself: ``--wav FILE --photo_landmarks TXT`` (or ``--photo_landmarks_from photo --fan_weights CKPT``, which detects them on the
aligned picture on the device: landmarks.py) runs the audio half of main_end2end_module2.py:181-272 in process -- mel
windows (audio.py) -> the two Module1 networks (``--load_a2l_G_name`` / ``--load_a2l_C_name`` checkpoints) -> the landmark
post-processing -> image-pixel landmarks -- with the photo's detected (68, 3) landmarks (``face_alignment`` output, a txt of 68
rows) and a speaker embedding as inputs: ``--speaker_emb`` txt of 256 numbers, or ``--speaker_emb_from wav --speaker_encoder
CKPT``, which embeds ``--wav`` on the device (speaker.py: resemblyzer's encoder restated, without its silence trim).  The matte comes from ``--matte PNG`` (white = foreground) unless the model has its matting network.
"""
import argparse
import os
import shutil
import subprocess
import sys

import numpy as np
import torch

from . import stream
from .models import create_model
from .options.base_options import TestOptions


def tensor2im(t):
    """util/util.py:9-29 for one (C, H, W) frame in [-1, 1] -> uint8 (H, W, 3)."""
    a = t.detach().float().cpu().numpy()
    if a.shape[0] == 1:
        a = np.tile(a, (3, 1, 1))
    elif a.shape[0] == 2:
        a = np.concatenate([a, a[1:2]], 0)
    return ((np.transpose(a, (1, 2, 0)) + 1) / 2.0 * 255.0).astype(np.uint8)


def load_photo(path, size, align='none', mtcnn_weights=None):
    """``align='mtcnn'``: the photo is first aligned in process as the reference's align_mtcnn does (animateportrait_amd.mtcnn)"""
    from PIL import Image
    im = Image.open(path).convert('RGB')
    if align == 'mtcnn':
        from . import mtcnn
        aligned = mtcnn.Detector(mtcnn_weights or mtcnn.DEFAULT_WEIGHTS).align_photo(np.asarray(im))
        if aligned is None:
            raise SystemExit('--align mtcnn: no face found in %s' % path)
        im = Image.fromarray(aligned)
    if im.size != (size, size):
        im = im.resize((size, size), Image.BICUBIC)
    a = np.asarray(im, dtype=np.float32) / 255.0
    return torch.from_numpy(a).permute(2, 0, 1).unsqueeze(0) * 2 - 1                # transforms.Normalize(0.5, 0.5)


def load_matte(path, size):
    from PIL import Image
    im = Image.open(path).convert('L')
    if im.size != (size, size):
        im = im.resize((size, size), Image.BILINEAR)
    return torch.from_numpy(np.asarray(im, dtype=np.float32) / 255.0).view(1, 1, size, size)


def aligned_photo_u8(a):
    """the 512 x 512 aligned picture the photo's landmarks are detected on (main_end2end_module2.py:186-193 detects on the
    picture align_mtcnn wrote): the result of --align mtcnn, or --photo itself, which must then be that picture"""
    from PIL import Image
    im = np.asarray(Image.open(a.photo).convert('RGB'))
    if a.align == 'mtcnn':
        from . import mtcnn
        im = mtcnn.Detector(a.mtcnn_weights or mtcnn.DEFAULT_WEIGHTS).align_photo(im)
        if im is None:
            raise SystemExit('--align mtcnn: no face found in %s' % a.photo)
    if im.shape[:2] != (512, 512):
        raise SystemExit('--photo_landmarks_from photo with --align none: --photo is the aligned 512 x 512 picture, got %d x %d'
                         % (im.shape[1], im.shape[0]))
    return im


def photo_landmarks_from_photo(a, device):
    """the (68, 3) landmarks of the aligned picture, detected on the device (landmarks.py: FAN of --fan_weights)"""
    from . import fan, landmarks
    det = landmarks.PhotoLandmarks(fan.load_fan(a.fan_weights, device), device, mtcnn_weights=a.mtcnn_weights)
    return det.detect(aligned_photo_u8(a), a.face_box).astype(np.float64)


def landmarks_from_audio(a, device):
    """main_end2end_module2.py:205-272 in process (mel -> AutoVC conversion -> both Module1 networks -> post-processing), with
    the clip's f0 track and speaker embedding as inputs: returns (photo landmarks (68, 2), clip (T, 68, 2)) px.  With
    --module1_post device the clip is a CUDA tensor that never was on the host."""
    from . import audio, module1
    if getattr(a, 'photo_landmarks_from', None) == 'photo':
        shape = photo_landmarks_from_photo(a, device)
    else:
        shape = np.loadtxt(a.photo_landmarks).reshape(68, -1)
    if shape.shape[1] == 2:
        shape = np.concatenate([shape, np.zeros((68, 1))], 1)
    std_z = np.loadtxt(a.std_face).reshape(68, 3)[:, 2] if a.std_face else None
    face_id, scale, shift = module1.adjust_and_norm_input_face(shape, std_z)
    net_g, net_c = module1.load_module1(a.load_a2l_G_name, a.load_a2l_C_name, device)
    if a.module1_lstm is not None:
        module1.set_lstm_backend(a.module1_lstm)
    if a.module1_post is not None:
        module1.set_post_backend(a.module1_post)
    if getattr(a, 'module1_encoder', None) is not None:
        module1.set_encoder_backend(a.module1_encoder)
    if a.speaker_emb_from == 'wav':
        # main_end2end_module2.py:216-219: the clip's own embedding, before the converter; it conditions both stages below
        from . import speaker
        x, sr = audio.read_wav(a.wav)
        emb = speaker.speaker_embedding(x, sr, speaker.load_encoder(a.speaker_encoder, device))
    else:
        emb = np.loadtxt(a.speaker_emb).reshape(-1).astype(np.float32)
    frontend = getattr(a, 'audio_frontend', None) or os.environ.get('APAMD_AUDIO_FRONTEND') or 'host'
    if frontend not in ('host', 'device'):
        raise ValueError("end2end: audio front end %r (known: 'host', 'device')" % (frontend,))
    clip = None
    if frontend == 'device':
        # one read_wav, one upload; the mel, the f0 tracker and Module1's windows all start from this object (audio_device.py)
        from . import audio_device
        clip = audio_device.ClipAudio(a.wav, device=device)
    converter = None
    if not a.no_autovc:
        # main_end2end_module2.py:218-224: Module1 sees the AutoVC-converted spectrogram, not the raw mel
        from . import autovc
        G = autovc.load_generator(a.load_AUTOVC_name, device)
        emb_trg = autovc.load_target_embedding(a.autovc_target_emb)
        f0 = np.load(a.f0_npy) if a.f0_npy else None
        if a.f0 == 'device':
            # the track of the samples clip_audio_features conditions: read, resample, loudness (f0.py conditions them itself)
            from . import f0 as f0_device
            if clip is not None:
                f0 = f0_device.f0_track(clip, a.f0_gender, device)
            else:
                x, sr = audio.read_wav(a.wav)
                f0 = f0_device.f0_track(audio.normalize_loudness(audio.resample_to_16k(x, sr)), a.f0_gender, device)
        if f0 is None:
            print('WARNING: no --f0_npy: the converter runs on an all-unvoiced f0 track (the reference extracts RAPT f0 with '
                  'pysptk, which is not in this image)')
        converter = lambda mel: autovc.convert_mel(G, mel, None if f0 is None else f0[:mel.shape[0]], emb, emb_trg, device)   # noqa: E731
    if clip is not None:
        windows = audio_device.clip_audio_features(clip, max_frames=a.max_frames, converter=converter, au_mean_std=getattr(a, 'au_mean_std', None))
    else:
        windows = audio.clip_audio_features(a.wav, max_frames=a.max_frames, converter=converter, au_mean_std=getattr(a, 'au_mean_std', None))
    fl = module1.predict_landmarks_speaker_aware(net_g, net_c, windows, emb, face_id.reshape(-1),
                                                 centerize_face=bool(getattr(a, 'centerize_face', False)),
                                                 no_y_rotation=bool(getattr(a, 'no_y_rotation', False)))
    seq = module1.to_image_landmarks(fl, scale=scale, shift=shift)[:, :, :2]
    if torch.is_tensor(seq):
        return module1.photo_landmarks_in_pixels(face_id, scale, shift), seq.contiguous()
    return module1.photo_landmarks_in_pixels(face_id, scale, shift), seq.astype(np.float32)


def make_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--photo', required=True)
    ap.add_argument('--align', choices=('none', 'mtcnn'), default='none',
                    help='mtcnn: detect the face and cut the aligned 512 x 512 picture from --photo on the device before anything '
                         'else reads it (align_mtcnn, main_end2end_module2.py:12-45); none: --photo is already aligned')
    ap.add_argument('--mtcnn_weights', default=None, help='with --align mtcnn: pnet.npy / rnet.npy / onet.npy directory or .npz '
                                                          '(default: MTCNN/weights)')
    ap.add_argument('--landmarks', default=None, help='directory in the Alm_txt layout')
    ap.add_argument('--landmarks_npy', default=None)
    ap.add_argument('--landmark_scale', type=float, default=1.0)
    ap.add_argument('--matte', default=None)
    ap.add_argument('--out', required=True)
    ap.add_argument('--fps', type=float, default=62.5)                              # main_end2end_module2.py:343
    ap.add_argument('--audio', default=None)
    ap.add_argument('--wav', default=None, help='drive the clip from this audio file (needs --photo_landmarks)')
    ap.add_argument('--photo_landmarks', default=None, help='txt, 68 rows "x y z": the photo\'s detected landmarks in pixels')
    ap.add_argument('--photo_landmarks_from', choices=('txt', 'photo'), default='txt',
                    help='where the photo\'s landmarks come from: txt = the file --photo_landmarks names, photo = detected on the '
                         'aligned 512 x 512 picture on the GPU (landmarks.py: face_alignment\'s FAN restated, fed the --align mtcnn '
                         'result, or --photo itself with --align none) with the checkpoint --fan_weights names')
    ap.add_argument('--fan_weights', default=None, help="with --photo_landmarks_from photo: face_alignment's 3D-FAN checkpoint")
    ap.add_argument('--face_box', type=_face_box, default=None,
                    help='with --photo_landmarks_from photo: x0,y0,x1,y1 of the face in the aligned picture (default: the MTCNN '
                         'detector\'s best face)')
    ap.add_argument('--speaker_emb', default=None, help='txt with the 256-d resemblyzer speaker embedding of the clip (required with --wav)')
    ap.add_argument('--speaker_emb_from', choices=('txt', 'wav'), default=None,
                    help='where the speaker embedding comes from: txt = the file --speaker_emb names, wav = computed from --wav on the '
                         'GPU with the encoder --speaker_encoder names (speaker.py, libapseq.so; long silences are not trimmed as '
                         'resemblyzer trims them); default: txt')
    ap.add_argument('--speaker_encoder', default=None, help="with --speaker_emb_from wav: resemblyzer's pretrained.pt")
    ap.add_argument('--load_AUTOVC_name', default='Module1/checkpoints/ckpt_autovc.pth',
                    help='AutoVC converter checkpoint (main_end2end_module2.py:43); Module1 is fed the converted spectrogram')
    ap.add_argument('--autovc_target_emb', default=None, help='target-speaker embedding txt (default: the reference checkout\'s obama_emb.txt)')
    ap.add_argument('--f0_npy', default=None, help='normalised RAPT f0 track of the clip (extract_f0_func_audiofile), one value per mel frame')
    ap.add_argument('--f0', choices=('npy', 'device'), default=None,
                    help='where the converter\'s f0 track comes from: npy = the file --f0_npy names, device = tracked from --wav on '
                         'the GPU (f0.py: RAPT as published, libapseq.so); default: --f0_npy when given, else an all-unvoiced track')
    ap.add_argument('--f0_gender', choices=('F', 'M'), default='F',
                    help='with --f0 device: the search range, F = 100 .. 600 Hz (what the reference\'s converter passes), M = 50 .. 250 Hz')
    ap.add_argument('--no_autovc', action='store_true',
                    help='feed the RAW mel spectrogram to Module1 (NOT what the reference does: its checkpoints were trained on '
                         'AutoVC-converted spectrograms); for experiments with networks trained that way')
    ap.add_argument('--std_face', default=None, help='STD_FACE_LANDMARKS.txt (its depth column replaces the detected one)')
    ap.add_argument('--centerize_face', action='store_true',
                    help='head stabilisation (train_audio2landmark.py:312-317): move every predicted frame\'s 68-point mean onto '
                         'that of the photo\'s normalised face (default: off)')
    ap.add_argument('--no_y_rotation', action='store_true',
                    help='head stabilisation (train_audio2landmark.py:319-338; the reference\'s name): register every predicted '
                         'frame\'s nose-and-eye-corner T shape onto the photo\'s and take one Euler angle out of the head\'s '
                         'rotation R = Rz(c) Ry(b) Rx(a).  The angle removed is a, the rotation about the x axis (the nod), not the '
                         'one about y the name promises: the reference zeroes the first entry of scipy\'s extrinsic \'xyz\' triple.  '
                         'With --module1_post device one launch of libapseq.so, else numpy / scipy (default: off)')
    ap.add_argument('--load_a2l_G_name', default='Module1/checkpoints/ckpt_speaker_branch.pth')
    ap.add_argument('--load_a2l_C_name', default='Module1/checkpoints/ckpt_content_branch.pth')
    ap.add_argument('--module1_lstm', choices=('library', 'hip'), default=None,
                    help='who runs the LSTMs of the two Module1 networks: library = nn.LSTM, hip = the batched kernel of '
                         'libapseq.so, one launch per layer (default: library, or what APAMD_MODULE1_LSTM names)')
    ap.add_argument('--module1_encoder', choices=('library', 'hip'), default=None,
                    help='who runs the self-attention encoder of Module1\'s pose network: library = the torch modules, hip = two '
                         'launches per layer of libapseq.so (default: library, or what APAMD_MODULE1_ENCODER names)')
    ap.add_argument('--au_mean_std', default=None,
                    help='table of mel means and standard deviations (the reference\'s MEAN_STD_AUTOVC_RETRAIN_MEL_AU.txt: 80 means, '
                         'then 80 standard deviations): Module1 is fed (mel - mean) / std of the converted spectrogram, as the '
                         'reference\'s test-time dataset feeds it (default: none, the unnormalised mel)')
    ap.add_argument('--module1_post', choices=('host', 'device'), default=None,
                    help='where Module1\'s landmark post-processing runs (Savitzky-Golay filters, baseline calibration, lip fixes, '
                         'eye lids): host = numpy / scipy, device = libapseq.so, the landmark sequence then stays on the GPU; with '
                         '--triangulate device it never leaves it (default: host, or what APAMD_MODULE1_POST names)')
    ap.add_argument('--audio_frontend', choices=('host', 'device'), default=None,
                    help='where --wav is resampled, normalised, filtered and turned into mel windows: host = numpy / scipy '
                         '(audio.py), device = libapseq.so (audio_device.py): the samples are uploaded once and the converter, '
                         '--f0 device and Module1 read device tensors (default: host, or what APAMD_AUDIO_FRONTEND names)')
    ap.add_argument('--max_frames', type=int, default=None)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--style', choices=('drawing', 'cartoon'), default='drawing',
                    help='cartoon: the model options of the cartoon experiment (--name formal/cartoon --output_nc 3, '
                         'main_end2end_module2.py:100-103; both can still be given explicitly); frames have three channels')
    ap.add_argument('--triangulate', choices=('host', 'device'), default='host',
                    help='where the motion grids\' Delaunay triangulation runs: scipy on the CPU per frame, or ap_delaunay on the GPU '
                         '(the landmark sequence is then uploaded once and no per-frame work is left on the host)')
    ap.add_argument('--png_encoder', choices=('host', 'device'), default='host',
                    help='who makes the frame PNGs: PIL on the host, one frame at a time, or apd_png_encode on the GPU in batches '
                         'of --batch (the same pixels in larger files; the host only writes them)')
    ap.add_argument('--png_channels', type=int, choices=(1, 3), default=3,
                    help='with --png_encoder device: 3 = RGB files as the host writes them, 1 = greyscale files (1-channel frames only)')
    ap.add_argument('--video', choices=('ffmpeg', 'avi'), default='ffmpeg',
                    help='ffmpeg: assemble the frame PNGs with an ffmpeg binary when one is found (output.mp4).  avi: encode the '
                         'frames as baseline JPEG on the GPU (apd_jpeg_encode) and write <out>/output.avi -- MJPG video with the PCM '
                         'sound of --audio / --wav -- in this process; no external tool is used')
    ap.add_argument('--video_quality', type=int, default=90, help='with --video avi: JPEG quality 1..100 (the IJG scale PIL uses)')
    ap.add_argument('--video_channels', type=int, choices=(1, 3), default=None,
                    help='with --video avi: 1 = greyscale JPEG (1-channel frames only), 3 = Y Cb Cr 4:4:4; default: 1 for 1-channel '
                         'frames, otherwise 3')
    ap.add_argument('--frames', choices=('png', 'none'), default='png',
                    help='none: write no per-frame PNG (only with --video avi)')
    ap.add_argument('--landmark_video', choices=('none', 'avi'), default='none',
                    help='avi: also write <out>/landmark_seq2.avi, the landmark sequence that drives the clip drawn as coloured face '
                         'contours on white (apd_landmark_vis on the GPU), at --fps with the sound of --audio / --wav')
    ap.add_argument('--landmark_video_size', type=_landmark_video_size, default=512,
                    help='with --landmark_video avi: side of its square frames, 256 .. 1024 (lines are 2 (size // 256) px thick)')
    ap.add_argument('--landmark_video_quality', type=int, default=90, help='with --landmark_video avi: JPEG quality 1..100')
    ap.add_argument('--side_outputs', action='store_true',
                    help='also write <out>/photo.png (the photo at --size) and <out>/ori_view.png (the photo with a red disc on each '
                         'of its landmarks), through --png_encoder')
    return ap


def _face_box(text):
    from .landmarks import parse_box
    return parse_box(text)


def _landmark_video_size(text):
    size = int(text)
    if not 256 <= size <= 1024:
        raise argparse.ArgumentTypeError('%d, served: 256 .. 1024 (below 256 the line thickness 2 (size // 256) is 0)' % size)
    return size


def write_avi_batches(batches, path, width, height, fps, audio=None, channels=3, quality=90, slot='clip'):
    """batches: an iterable of (n, C, height, width) device tensors, made one at a time -> an AVI file of MJPG frames
    (util/avi.py) with the PCM sound of the wav `audio`.  A batch is encoded where it is (data/visuals.encode_jpeg_batch) into
    two pinned buffers in turn, and a writer thread appends it to the file while the next is made and encoded: the pattern of
    write_frames.  Only the batch in hand is alive, so a clip never has to exist as a whole."""
    import concurrent.futures
    from .data import visuals
    from .util import avi
    num, den = avi.fps_fraction(fps)
    writer = avi.AviWriter(path, width, height, num, den, audio=audio)
    pending = None
    with concurrent.futures.ThreadPoolExecutor(max_workers=1) as pool:
        try:
            for turn, frames in enumerate(batches):
                buf, sizes = visuals.encode_jpeg_batch(frames, channels=channels, quality=quality, slot='%s%d' % (slot, turn & 1))
                done = torch.cuda.Event()
                done.record()
                if pending is not None:
                    pending.result()          # the other buffer is in the file before it is encoded into again (next turn)
                done.synchronize()
                pending = pool.submit(writer.add_frames, buf, sizes)
            if pending is not None:
                pending.result()
        finally:
            writer.close()
    return writer.frames


def write_avi(frames, path, fps, audio=None, batch=16, channels=None, quality=90):
    """frames (T, C, H, W) -> an AVI file, --batch frames at a time through write_avi_batches."""
    if not frames.is_cuda:
        frames = frames.cuda()
    if channels is None:
        channels = 1 if frames.shape[1] == 1 else 3
    return write_avi_batches((frames[k0:k0 + batch] for k0 in range(0, frames.shape[0], batch)), path, frames.shape[3],
                             frames.shape[2], fps, audio, channels, quality)


def truncated_landmarks(seq, scale):
    """(T, P, 2) float landmarks scaled and made int32 as vis_landmark makes them (main_end2end_module2.py:49: astype('int32'),
    truncation toward zero); NaN goes to 0 and anything beyond +-2^20 to that bound, where the cast is still defined."""
    a = np.nan_to_num(np.asarray(seq, dtype=np.float64) * scale, nan=0.0)
    return np.clip(a, -2.0 ** 20, 2.0 ** 20).astype(np.int32)


def write_landmark_avi(seq, path, fps, device, audio=None, batch=16, size_in=256, size_out=512, quality=90):
    """The predicted landmark sequence as coloured face contours on white, the counterpart of landmark_seq2.mov
    (main_end2end_module2.py:281, 303): seq (T, 68, 2) in pixels of a size_in frame -> MJPG frames of size_out x size_out.  The
    integer landmarks are uploaded once; a batch of frames is drawn by one apd_landmark_vis launch when the encoder asks for it."""
    from .data import visuals
    table = visuals.FACE_CONTOURS
    thickness, radius = visuals.face_contour_style(size_out)
    pts = torch.from_numpy(truncated_landmarks(seq, size_out / float(size_in))).to(device)

    def batches():
        for k0 in range(0, pts.shape[0], batch):
            yield visuals.landmark_vis(pts[k0:k0 + batch], table['segments'], table['colours'], size_out, size_out, radius, thickness,
                                       table['disc_rgb'])
    with torch.cuda.device(device):
        return write_avi_batches(batches(), path, size_out, size_out, fps, audio, 3, quality, slot='landmarks')


def write_side_outputs(photo, lm0, out_dir, device, encoder='host'):
    """<out_dir>/photo.png: the photo as the generator sees it; <out_dir>/ori_view.png: the same with a red disc on every photo
    landmark (main_end2end_module2.py:286, 328-331 draws radius 5 at 512 px: round(5 size / 512) here), coordinates by Python's round."""
    from .data import visuals
    size = photo.shape[-1]
    photo = photo.to(device).float().contiguous()
    pts = np.clip(np.rint(np.nan_to_num(np.asarray(lm0, dtype=np.float64)[:, :2])), -2.0 ** 20, 2.0 ** 20).astype(np.int32)[None]
    marked = visuals.landmark_vis(pts, None, None, size, size, round(5 * size / 512), 1, visuals.FACE_CONTOURS['disc_rgb'], bg=photo)
    names = {'photo': [os.path.join(out_dir, 'photo.png')], 'ori_view': [os.path.join(out_dir, 'ori_view.png')]}
    with torch.cuda.device(device):
        return visuals.save_png_batch({'photo': photo, 'ori_view': marked}, names, encoder=encoder)


def write_frames(frames, fdir, encoder='host', batch=16, channels=3):
    """frames (T, C, H, W) -> <fdir>/%05d.png.  'host': tensor2im + PIL per frame.  'device': the frames are encoded where they
    are, --batch at a time (data/visuals.encode_png_batch), two pinned buffers in turn so that a batch is written to disk while
    the next is encoded."""
    if encoder == 'host':
        from PIL import Image
        for k in range(frames.shape[0]):
            Image.fromarray(tensor2im(frames[k])).save(os.path.join(fdir, '%05d.png' % k))
        return
    from .data import visuals
    if not frames.is_cuda:
        frames = frames.cuda()

    def write(job):
        with open(job[1], 'wb') as f:
            f.write(job[0])
    pending = None
    for turn, k0 in enumerate(range(0, frames.shape[0], batch)):
        buf, sizes = visuals.encode_png_batch(frames[k0:k0 + batch], channels=channels, slot='clip%d' % (turn & 1))
        done = torch.cuda.Event()
        done.record()
        if pending is not None:
            list(pending)                 # the other buffer's files are on disk before it is encoded into again (next turn)
        done.synchronize()
        pending = visuals.png_pool().map(write, [(buf.numpy()[i, :size], os.path.join(fdir, '%05d.png' % (k0 + i)))
                                                 for i, size in enumerate(sizes.tolist())])
    if pending is not None:
        list(pending)


def main(argv=None, prepare_model=None):
    """``prepare_model(model)`` runs after the model is built and before setup(), as in test.main: the place to attach the frozen
    third-party networks (aux['netF'], aux['modnet'])."""
    ap = make_parser()
    a, rest = ap.parse_known_args(argv)
    if sum(x is not None for x in (a.landmarks, a.landmarks_npy, a.wav)) != 1:
        ap.error('exactly one of --landmarks / --landmarks_npy / --wav')
    if a.photo_landmarks_from == 'photo':
        if a.photo_landmarks is not None:
            ap.error('--photo_landmarks_from photo detects the landmarks on the picture: it does not go with --photo_landmarks')
        if a.wav is None:
            ap.error('--photo_landmarks_from photo needs --wav')
        if a.fan_weights is None:
            ap.error('--photo_landmarks_from photo needs --fan_weights (face_alignment\'s 3D-FAN checkpoint)')
    elif a.fan_weights is not None:
        ap.error('--fan_weights goes with --photo_landmarks_from photo')
    elif a.face_box is not None:
        ap.error('--face_box goes with --photo_landmarks_from photo')
    if a.wav is not None and a.photo_landmarks is None and a.photo_landmarks_from != 'photo':
        ap.error('--wav needs --photo_landmarks (or --photo_landmarks_from photo)')
    if a.speaker_emb_from == 'wav':
        if a.speaker_emb is not None:
            ap.error('--speaker_emb_from wav computes the embedding from --wav: it does not go with --speaker_emb')
        if a.wav is None:
            ap.error('--speaker_emb_from wav needs --wav')
        if a.speaker_encoder is None:
            ap.error('--speaker_emb_from wav needs --speaker_encoder (resemblyzer\'s pretrained.pt)')
    elif a.speaker_encoder is not None:
        ap.error('--speaker_encoder goes with --speaker_emb_from wav')
    if a.wav is not None and a.speaker_emb is None and a.speaker_emb_from != 'wav':
        ap.error('--wav needs --speaker_emb (the 256-d resemblyzer embedding the speaker-aware branch is conditioned on, '
                 'main_end2end_module2.py:215-217); a zero vector is not a neutral default')
    if a.f0 == 'device' and a.f0_npy is not None:
        ap.error('--f0 device tracks the f0 from --wav: it does not go with --f0_npy')
    if a.f0 == 'npy' and a.f0_npy is None:
        ap.error('--f0 npy needs --f0_npy')
    if a.f0 == 'device' and (a.wav is None or a.no_autovc):
        ap.error('--f0 device: the track feeds the AutoVC converter of --wav (it needs --wav, without --no_autovc)')
    if a.frames == 'none' and a.video != 'avi':
        ap.error('--frames none leaves nothing to assemble: it needs --video avi')
    if not 1 <= a.video_quality <= 100:
        ap.error('--video_quality %d, served: 1 .. 100' % a.video_quality)
    if not 1 <= a.landmark_video_quality <= 100:
        ap.error('--landmark_video_quality %d, served: 1 .. 100' % a.landmark_video_quality)
    if a.wav is not None and not a.no_autovc and not os.path.exists(a.load_AUTOVC_name):
        ap.error('--wav: AutoVC checkpoint %s not found; the reference converts the spectrogram before Module1 '
                 '(pass --load_AUTOVC_name, or --no_autovc to feed the raw mel on purpose)' % a.load_AUTOVC_name)
    # the model's own options: the test settings of test_gan_new (:95-104) unless given
    defaults = ['--model', 'geomcgt_ifw_test', '--netG', 'resnet_9blocks_rcatland32_full_ifw', '--netg_resb_div', '3',
                '--netg_resb_disp', '3', '--output_nc', '1', '--dataset_mode', 'synthetic', '--blendbg', '1', '--gpu_ids', '0']
    if a.style == 'cartoon':
        # the model takes the cartoon branch for experiment names that contain 'cartoon' (geomcgt_ifw_test_model.py:228)
        defaults += ['--output_nc', '3', '--name', 'formal/cartoon']          # (argparse keeps the last value of an option)
    opt = TestOptions().parse(defaults + rest)
    if a.style == 'cartoon' and 'cartoon' not in opt.name:
        ap.error('--style cartoon with --name %s: the cartoon branch is selected by an experiment name that contains "cartoon"' % opt.name)
    torch.cuda.set_device(opt.gpu_ids[0])
    model = create_model(opt)
    if prepare_model is not None:
        prepare_model(model)
    model.setup(opt)                    # '<epoch>_net_G_A.pth' + the static drawing generator; missing files are errors
    model.eval()
    if a.wav is not None:
        lm0, seq = landmarks_from_audio(a, torch.device('cuda', opt.gpu_ids[0]))
        if a.audio is None:
            a.audio = a.wav
    elif a.landmarks is not None:
        lm0, seq = stream.load_landmark_dir(a.landmarks, a.landmark_scale)
    else:
        arr = np.load(a.landmarks_npy).astype(np.float32) * a.landmark_scale
        lm0, seq = arr[0], arr[1:]
    photo = load_photo(a.photo, a.size, a.align, a.mtcnn_weights)
    matte = load_matte(a.matte, a.size) if a.matte else None
    if matte is None and model.aux.get('modnet') is None:
        raise SystemExit('no matting network is attached (aux["modnet"]): pass --matte PNG')
    # the previews come first: they show what the generator is about to be given, whatever becomes of the clip
    device = torch.device('cuda', opt.gpu_ids[0])
    if a.side_outputs:
        os.makedirs(a.out, exist_ok=True)
        write_side_outputs(photo, lm0, a.out, device, a.png_encoder)
        print('wrote photo.png and ori_view.png to', a.out)
    if a.landmark_video == 'avi':
        os.makedirs(a.out, exist_ok=True)
        preview = os.path.join(a.out, 'landmark_seq2.avi')
        write_landmark_avi(seq.cpu() if torch.is_tensor(seq) else seq, preview, a.fps, device, a.audio, a.batch, a.size, a.landmark_video_size, a.landmark_video_quality)
        print('landmark preview is', preview)
    if torch.is_tensor(seq) and seq.is_cuda and a.triangulate == 'host':
        seq = seq.cpu()                  # scipy triangulates per frame on the host: the sequence crosses once, here
    frames = stream.ClipStreamer(model, batch=a.batch, triangulate=a.triangulate).run(photo, lm0, seq, matte=matte)
    fdir = os.path.join(a.out, 'frames')
    if a.frames == 'png':
        os.makedirs(fdir, exist_ok=True)
        write_frames(frames, fdir, a.png_encoder, a.batch, a.png_channels)
        print('wrote %d frames to %s' % (frames.shape[0], fdir))
    if a.video == 'avi':
        os.makedirs(a.out, exist_ok=True)
        video = os.path.join(a.out, 'output.avi')
        write_avi(frames, video, a.fps, a.audio, a.batch, a.video_channels, a.video_quality)
        print('output is', video)
        return 0
    ffmpeg = shutil.which('ffmpeg')
    if ffmpeg is None:
        print('ffmpeg not found: frames only (the reference assembles them at %.1f fps, :118-121)' % a.fps)
        return 0
    video = os.path.join(a.out, 'output.mp4')
    subprocess.check_call([ffmpeg, '-loglevel', 'panic', '-framerate', str(a.fps), '-i', os.path.join(fdir, '%05d.png'),
                           '-c:v', 'libx264', '-y', '-vf', 'format=yuv420p', video])
    if a.audio:
        subprocess.check_call([ffmpeg, '-loglevel', 'panic', '-i', video, '-i', a.audio, '-vcodec', 'copy', '-acodec', 'copy',
                               '-y', video.replace('.mp4', '.mov')])
    print('output is', video)
    return 0


if __name__ == '__main__':
    sys.exit(main())
