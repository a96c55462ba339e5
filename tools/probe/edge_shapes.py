import sys, os
sys.path.insert(0, "vision-transformers-pytorch_amd")
import torch
from models import SwinTransformer, VisionTransformer
from models.halo_transformer import HaloTransformer
from models.twins import TwinsSVT
from vtx.nn import Linear
dev = torch.device("cuda")
def run(name, f):
    try:
        out = f()
        print(name, "OK", tuple(out.shape), bool(torch.isfinite(out.float()).all()))
    except Exception as e:
        print(name, "->", type(e).__name__, str(e)[:160])
with torch.autocast("cuda", dtype=torch.bfloat16):
    run("swin 448 win7", lambda: SwinTransformer(image_size=(448, 448), n_class=16, depths=(1,1,1,1), dims=(32,64,128,256), dim_head=32, n_heads=(1,2,4,8), dim_ffs=(64,128,256,512), window_size=7).to(dev)(torch.randn(2,3,448,448,device=dev)))
    run("swin 384 win12", lambda: SwinTransformer(image_size=(384, 384), n_class=16, depths=(1,1,1,1), dims=(32,64,128,256), dim_head=32, n_heads=(1,2,4,8), dim_ffs=(64,128,256,512), window_size=12).to(dev)(torch.randn(2,3,384,384,device=dev)))
    run("swin 224x448", lambda: SwinTransformer(image_size=(224, 448), n_class=16, depths=(1,1,1,1), dims=(32,64,128,256), dim_head=32, n_heads=(1,2,4,8), dim_ffs=(64,128,256,512), window_size=7).to(dev)(torch.randn(2,3,224,448,device=dev)))
    # window / halo attention at other head widths and windows: csrc/attention_hd.hip behind vtx_attn_hdw_*
    run("swin dim_head 16", lambda: SwinTransformer(image_size=(224, 224), n_class=16, depths=(1,1,1,1), dims=(32,64,128,256), dim_head=16, n_heads=(2,4,8,16), dim_ffs=(64,128,256,512), window_size=7).to(dev)(torch.randn(2,3,224,224,device=dev)))
    run("swin dim_head 48", lambda: SwinTransformer(image_size=(224, 224), n_class=16, depths=(1,1,1,1), dims=(96,192,384,768), dim_head=48, n_heads=(2,4,8,16), dim_ffs=(192,384,768,1536), window_size=7).to(dev)(torch.randn(2,3,224,224,device=dev)))
    run("swin 416 win13 (169 tokens)", lambda: SwinTransformer(image_size=(416, 416), n_class=16, depths=(1,1,1,1), dims=(32,64,128,256), dim_head=32, n_heads=(1,2,4,8), dim_ffs=(64,128,256,512), window_size=13).to(dev)(torch.randn(2,3,416,416,device=dev)))
    run("swin 448 win14 dim_head 64 (196 tokens)", lambda: SwinTransformer(image_size=(448, 448), n_class=16, depths=(1,1,1,1), dims=(64,128,256,512), dim_head=64, n_heads=(1,2,4,8), dim_ffs=(128,256,512,1024), window_size=14).to(dev)(torch.randn(2,3,448,448,device=dev)))
    run("twins local dim_head 16", lambda: TwinsSVT(n_class=16, depths=(1,1,1,1), dims=(32,64,128,256), dim_head=16, n_heads=(2,4,8,16), dim_ffs=(64,128,256,512), window_size=7).to(dev)(torch.randn(2,3,224,224,device=dev)))
    run("halo dim_head 16", lambda: HaloTransformer(image_size=(224, 224), n_class=16, depths=(1,1,1,1), dims=(64,128,256,512), dim_head=16, n_heads=(2,4,8,16), dim_ffs=(128,256,512,1024), window_size=7, halo_size=3).to(dev)(torch.randn(2,3,224,224,device=dev)))
    run("swin dim_head 20 (refused)", lambda: SwinTransformer(image_size=(224, 224), n_class=16, depths=(1,1,1,1), dims=(40,80,160,320), dim_head=20, n_heads=(2,4,8,16), dim_ffs=(80,160,320,640), window_size=7).to(dev)(torch.randn(2,3,224,224,device=dev)))
    run("vit 384 (L=577)", lambda: VisionTransformer(Linear(128,16), 384, 16, 2, 128, 2, 256, 0.,0.,0.,0.).to(dev)(torch.randn(2,3,384,384,device=dev)))
    run("vit 160 (L=101)", lambda: VisionTransformer(Linear(128,16), 160, 16, 2, 128, 2, 256, 0.,0.,0.,0.).to(dev)(torch.randn(2,3,160,160,device=dev)))
    run("vit dim_head 32", lambda: VisionTransformer(Linear(128,16), 224, 16, 2, 128, 4, 256, 0.,0.,0.,0.).to(dev)(torch.randn(2,3,224,224,device=dev)))
    run("vit eval no_grad", lambda: VisionTransformer(Linear(128,16), 224, 16, 2, 128, 2, 256, 0.,0.,0.,0.).to(dev).eval()(torch.randn(2,3,224,224,device=dev)))
