import os, sys, json, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ffrnet_amd
from ffrnet_amd import synth
specs = json.load(open(os.path.join(ROOT, 'tests/golden/g0_state_dict_keys.json')))
eng = ffrnet_amd.Engine(0); eng.load_encoder(synth.synth_state_dict(specs['encoder']))
x = synth.synth_images(256, seed=1).cuda()
eng.encoder_trunk_nhwc(x, 24)
