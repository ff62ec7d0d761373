"""The rate of the path when the boundary hands over HOST 8-bit pixels (yk_upload_pixels_u8: interleaved RGBA rows -> HBM over PCIe, widened by
the unpack kernel) and takes the packed tile maps back to the host: the 8-bit counterpart of tools/pcie_inclusive.py, which hands over int32
planes.  Never the bench's `value`.  Then the same frame step by step (each step ends in a host synchronisation): the two uploads, the encode
with the export of the tile maps, and the copy of the maps back.  usage: python tools/pixels_in.py [size]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from yaik_amd.encoder import HipTileEncoder
from yaik_amd.synth import synth_planes_torch

W = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
planes = synth_planes_torch(W, n_planes=4, device="cuda")
host = planes.to(torch.uint8).permute(1, 2, 0).contiguous().cpu().numpy()      # [W, W, 4] RGBA
pinned = torch.from_numpy(host).pin_memory().numpy()
enc = HipTileEncoder(0)
enc.set_image_u8(host)
blob = torch.empty(enc.export_capacity(), dtype=torch.uint8, device="cuda")
for name, pixels in (("pageable host pixels", host), ("pinned host pixels", pinned)):
    for rep in range(3):
        t0 = time.perf_counter()
        enc.set_image_u8(pixels)                   # H2D copy of 4 B per pixel + the unpack kernel
        enc.alpha_reject(); enc.alpha_finish(None)
        enc.encode(3, False, False)
        sizes = enc.export_tile_maps(blob)         # packed tile maps (alpha bitmap, 7 tile bitmaps, 3 x defs, 3 x nibbles) in one device buffer
        n = int(sizes.sum())
        back = blob[:n].cpu()                      # ... and back on the host
        t1 = time.perf_counter()
    print(f"{name}: {1e3 * (t1 - t0):.2f} ms per {W}x{W} RGBA frame = {W * W / 1e6 / (t1 - t0):.0f} Mpix/s (upload {host.nbytes / 1e6:.0f} MB, maps back {n / 1e6:.1f} MB)", flush=True)
ms, k = enc.stage_ms(7)
print(f"unpack kernel (YK_STAGE_UNPACK, event-timed): {ms / k:.3f} ms per frame over {k} calls", flush=True)

host32 = planes.cpu().numpy()                      # the same frame as int32 planes, pageable: what tools/pcie_inclusive.py uploads
del planes
steps = {"upload 8-bit pixels (yk_upload_pixels_u8)": lambda: enc.set_image_u8(host),
         "upload int32 planes (yk_upload_planes)": lambda: enc.set_image(host32),
         "alpha + encode + export of the maps": lambda: (enc.alpha_reject(), enc.alpha_finish(None), enc.encode(3, False, False), enc.export_tile_maps(blob)),
         "maps back to the host": lambda: blob[:n].cpu()}
for name, fn in steps.items():
    best = None
    for rep in range(3):
        t0 = time.perf_counter()
        fn()
        enc.synchronize(); torch.cuda.synchronize()
        t1 = time.perf_counter()
        best = t1 - t0 if best is None else min(best, t1 - t0)
    print(f"step, pageable, best of 3: {name}: {1e3 * best:.2f} ms", flush=True)
