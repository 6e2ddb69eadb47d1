"""The host packers' output is pinned: for every case of scripts/make_pack_pins.py the sizes the library returns and the SHA-256 of the
packed host blob, as the commit before csrc/conv_layer.h (one layer constructor, one affine packer, one Conv3d plan) produced them.
PINS is that script's output at that commit, pasted.  Equality only: a pin that differs is a bug in the packing code, never a pin to
regenerate — a changed blob layout means pack and forward of every model have to be proved again."""
import importlib.util
import os

import pytest

_spec = importlib.util.spec_from_file_location(
    "make_pack_pins", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "make_pack_pins.py"))
pins = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(pins)

PINS = {
    'conv2d-1-128-3-3-bf16x3': {'packed_floats': 55328, 'sha256': '65f35da8c23245a39edd9c5a7f54cf81ef155af1101821ae91a18555cba8fa7b'},
    'conv2d-1-128-3-3-fp16x2': {'packed_floats': 36900, 'sha256': 'df0484107be814411c3711432bb3afb4ef0eb8cde111d5229861831379c36906'},
    'conv2d-1-128-3-3-fp32': {'packed_floats': 36896, 'sha256': '18416f7df5e2e637a91a00d556c83db8b27d8abc034dba36011a6c215eec5d04'},
    'conv2d-127-256-3-3-bf16x3': {'packed_floats': 442496, 'sha256': '4e89655a0bbd8dcbf4bf23e88cce20d1d9ff004d38574bcb0ed2611f7a231a3b'},
    'conv2d-127-256-3-3-fp16x2': {'packed_floats': 295044, 'sha256': 'b42cb4e2db5a7e455fb4bfb1393cc642eea93c294d55151f140a682c8cda1e2f'},
    'conv2d-127-256-3-3-fp32': {'packed_floats': 295040, 'sha256': 'faa0a4025967dd5879ab1383a9410b37ab29d0fc3e9b4284a8b13a9652f3ac26'},
    'conv2d-128-320-5-1-bf16x3': {'packed_floats': 307328, 'sha256': '5d23deb071a42e025249c9c397ad537e965524529913654abde704c93f5b8dc8'},
    'conv2d-128-320-5-1-fp16x2': {'packed_floats': 204932, 'sha256': '0ace3a2d583ecd4b85ae999c8eb5ecf223afec877a8124a1e7571f8b7d27bb68'},
    'conv2d-128-320-5-1-fp32': {'packed_floats': 204928, 'sha256': 'b3f90f4f5b962bb1aaae7f34d678b943b2ef462ae2675a7fbfb9549b53b2b72d'},
    'conv2d-192-256-3-3-bf16x3': {'packed_floats': 663744, 'sha256': '7de6a606ae42464e3caeb1d715bca42c2bea54a5937a9e88ff22336246eebc96'},
    'conv2d-192-256-3-3-fp16x2': {'packed_floats': 442564, 'sha256': '6520005b18c8b3e6161ed823a52d96716497993c6e9c58d9a3182d103b58cdad'},
    'conv2d-192-256-3-3-fp32': {'packed_floats': 442560, 'sha256': '96be668630d2b56ab9bec0d020673ed7111c70706740230b2ddf3ba5457a6470'},
    'conv2d-256-320-1-5-bf16x3': {'packed_floats': 614656, 'sha256': '30a28ef145fa2d6ed4c8ecb7ec0397c0edd4605e4ffb42c0bc80cbebea09d4fe'},
    'conv2d-256-320-1-5-fp16x2': {'packed_floats': 409860, 'sha256': 'e9b30fff318842e6218bff4413e71c56b9009b2e23965a8c72f7bc3b3c3aa43b'},
    'conv2d-256-320-1-5-fp32': {'packed_floats': 409856, 'sha256': '97df6acf633e0db06e7bc22c0faf2287ec317dfc3d205a29c829964f713d756f'},
    'conv2d-256-36-1-1-bf16x3': {'packed_floats': -1},
    'conv2d-256-36-1-1-fp16x2': {'packed_floats': -1},
    'conv2d-256-36-1-1-fp32': {'packed_floats': 16640, 'sha256': '2ea1f7a74116d43f8bde2f709cece14ff0cebc28c01122b728da6768f73ce8e0'},
    'conv2d-576-256-1-1-bf16x3': {'packed_floats': 221760, 'sha256': '85a8f52fd74e5534acd92b0b97f5883c3294751736e9621ff4cdb510f801edb9'},
    'conv2d-576-256-1-1-fp16x2': {'packed_floats': 148036, 'sha256': '9a503e48d547b7b3b1102a07daff712e861d09ba1e510cf0b45e68a3085f7dcf'},
    'conv2d-576-256-1-1-fp32': {'packed_floats': 148032, 'sha256': 'cd54a9f86e163f09780a02744980061bcfa0b081ba8ea4c3987c1e730dfdfc1d'},
    'conv3d-16-16-0-1-bf16x3': {'packed_floats': 55456, 'sha256': '1e74efa2e77b134b388180baa8bce7e8718fb8d71dc592866f4214c428c0fe3a'},
    'conv3d-16-16-0-1-fp16x2': {'packed_floats': 46548, 'sha256': '3a0c51f31a2e74b1e1a136b19ed295a4dae64b4006d2973cde9befab1e93b92d'},
    'conv3d-16-16-0-1-fp32': {'packed_floats': 39328, 'sha256': '743b88cc5868bd94aea61a0f9928b2db358adb60fcb4a4bcb86fa5852f281f68'},
    'conv3d-16-16-16-1-bf16x3': {'packed_floats': 110752, 'sha256': 'd3a85c14f0e9b6347bb7bab743144955fb5a42c27121b1227b770e579eb8ce94'},
    'conv3d-16-16-16-1-fp16x2': {'packed_floats': 92372, 'sha256': '73acdc277c8bc66718879b09a7870d28240b6fec7f51a636f46b2d9900db2a65'},
    'conv3d-16-16-16-1-fp32': {'packed_floats': 78496, 'sha256': '26d36943b5878f224bfcfc506dc961302eb73db912f6e3f9636221da76507655'},
    'conv3d-16-32-0-1-bf16x3': {'packed_floats': 110752, 'sha256': 'e6fccf26984a506a2a595587f3a9fbb2b2d612738a50da9095259d8567818638'},
    'conv3d-16-32-0-1-fp16x2': {'packed_floats': 92372, 'sha256': '55d73ee42c3b53d1e2d1882bee7edc14cf419afa2317268e6be51de643c9b7fc'},
    'conv3d-16-32-0-1-fp32': {'packed_floats': 78496, 'sha256': '8ebd4479bd895f3b240093536897ddf8229091dd0c63c4edbe4886f26e466e5c'},
    'conv3d-16-8-0-2-bf16x3': {'packed_floats': 12768, 'sha256': '46ba0fad91e7bd36c933b260afee6edae856299d2e27df571bf920d91aff1396'},
    'conv3d-16-8-0-2-fp16x2': {'packed_floats': 16388, 'sha256': '463d24a071f55f6cee386b380b2c907ed502239340328ccf1ddf52c91ffa1a16'},
    'conv3d-16-8-0-2-fp32': {'packed_floats': 12768, 'sha256': '46ba0fad91e7bd36c933b260afee6edae856299d2e27df571bf920d91aff1396'},
    'conv3d-32-16-0-2-bf16x3': {'packed_floats': 13888, 'sha256': '56c42b7b7013c18218c4f0e9af315b8959954cdd42c2f90be491c1b1c17463b6'},
    'conv3d-32-16-0-2-fp16x2': {'packed_floats': 28292, 'sha256': 'dbf6866cae14c597e5f2bfd7df554036f648926823c0a40d1f035eb81ad2abcb'},
    'conv3d-32-16-0-2-fp32': {'packed_floats': 13888, 'sha256': '56c42b7b7013c18218c4f0e9af315b8959954cdd42c2f90be491c1b1c17463b6'},
    'conv3d-32-32-0-1-bf16x3': {'packed_floats': 41536, 'sha256': 'e351cf5612b7fbcb9c1bf136d152aeaf127b4a5348e941881c70e9c61d665bca'},
    'conv3d-32-32-0-1-fp16x2': {'packed_floats': 27720, 'sha256': '9d8a018296880ac97a09907d60ad08909ff396068a55cbfacc89b7838493502a'},
    'conv3d-32-32-0-1-fp32': {'packed_floats': 27712, 'sha256': 'cbb9a6fe28ec7880a3e50fee89d566a97a6cd40562f6abba1a02a5889a736c2b'},
    'conv3d-32-32-32-1-bf16x3': {'packed_floats': 83008, 'sha256': '55d9f9dd67242aa0c1ab9ebc1a54825fd05042b0a9b623db5f90a0f9e9e8dfa1'},
    'conv3d-32-32-32-1-fp16x2': {'packed_floats': 55368, 'sha256': '29acaf61ae8df252cdbcfbf5efc66da562a16c52f59365e7548a684c2f48a90f'},
    'conv3d-32-32-32-1-fp32': {'packed_floats': 55360, 'sha256': '0ecdba2434af5bc309af297096794f742ef602cac3653d911e3039d5385802ee'},
    'conv3d-32-64-0-1-bf16x3': {'packed_floats': 83008, 'sha256': 'e8ef8662d76aff0f12554a1f4071c94f6cc00757d966948efe213fa7229644be'},
    'conv3d-32-64-0-1-fp16x2': {'packed_floats': 55368, 'sha256': '3dc9a612d6c3ca8bcf75f5d8c4a4a40f7272384a2da44ef440170870af068926'},
    'conv3d-32-64-0-1-fp32': {'packed_floats': 55360, 'sha256': '6d1c1559715e7602cb1410de929f295b73c166d85c96dac61a4ddb96b6e4b921'},
    'conv3d-64-32-0-2-bf16x3': {'packed_floats': 55424, 'sha256': '10383c178cc8cbaae65dea3854a00da02ff8690fa31f9a2a6fab5d4d5fa5e839'},
    'conv3d-64-32-0-2-fp16x2': {'packed_floats': 55424, 'sha256': '10383c178cc8cbaae65dea3854a00da02ff8690fa31f9a2a6fab5d4d5fa5e839'},
    'conv3d-64-32-0-2-fp32': {'packed_floats': 55424, 'sha256': '10383c178cc8cbaae65dea3854a00da02ff8690fa31f9a2a6fab5d4d5fa5e839'},
    'conv3d-64-64-0-1-bf16x3': {'packed_floats': 166016, 'sha256': 'cfe4c7dec5832170261b7eba19748dc793bcc57dd03986b26b687744584b83ed'},
    'conv3d-64-64-0-1-fp16x2': {'packed_floats': 110728, 'sha256': '6c3bb192a52baa9736dceb5fd5f1498b68e8d8db68260a5aaa3b96b7571ad536'},
    'conv3d-64-64-0-1-fp32': {'packed_floats': 110720, 'sha256': '5893a7b6b659d9e13a4518310e558a9ebee8a198efdcf7031f9a9fe32c2a21e8'},
    'conv3d-8-16-0-1-bf16x3': {'packed_floats': 65808, 'sha256': '946b29f186192f630190c05ca1d5afcf0194cba3740849b2ab9f2ab3268f9e48'},
    'conv3d-8-16-0-1-bf16x3-0-1': {'packed_floats': 65808, 'sha256': 'd665fa0ca43581165ddd08c247663e09af3aeecf922e6c43ec2c5aa8e97e63b6'},
    'conv3d-8-16-0-1-fp16x2': {'packed_floats': 54324, 'sha256': '6e9e3922a175a8d4ef04630b1da1dbe69b7e5e2e0a2a895956889abd9e1f8c88'},
    'conv3d-8-16-0-1-fp16x2-0-1': {'packed_floats': 54324, 'sha256': '3c5fe8cf311352c488f7c6e777775fbf1a3f2f16f95c1fb1770a740b75e36ea2'},
    'conv3d-8-16-0-1-fp32': {'packed_floats': 45072, 'sha256': '7ac4ca6bb538fb225f35ca9d1e65b5ab975d0f13f3e007afbd49fea660c798f5'},
    'conv3d-8-16-0-1-fp32-0-1': {'packed_floats': 45072, 'sha256': '23d1667c664ec1214f10d14d99782f70055ec68ce978e875ea26e601ee093cea'},
    'conv3d-8-8-0-1-bf16x3': {'packed_floats': 31824, 'sha256': '72a5853ca2b831d218994bdbca9b210f617b54d1421d0478e22a525a951081c3'},
    'conv3d-8-8-0-1-fp16x2': {'packed_floats': 29548, 'sha256': 'e253717ed8d35baebd53a8d493edd47ebb4d6925b8fc865b8d1bbb714b95a6d2'},
    'conv3d-8-8-0-1-fp32': {'packed_floats': 24912, 'sha256': '03cc0dddb453729a5d840b145c7ced952adf2e42664913c9a6aae3e0f4fe9d2a'},
    'conv_norm-96-64-1-1-0-0': {'packed_floats': 6336, 'sha256': '7b3c0645dea8140488154a2060739eb11693c0e4c187f2d2fff349e4c2a2f146'},
    'conv_norm-96-64-1-1-0-1': {'packed_floats': 6336, 'sha256': 'e44c95ce01430e23360d73443971861153e17f309ee870f6dc4251f25b945539'},
    'conv_norm-96-64-1-1-1-0': {'packed_floats': 6336, 'sha256': '4680a07dabbcefe89e8c450646e9696bcf01b647c171c706b4e96bf2a09b3553'},
    'conv_norm-96-64-1-1-1-1': {'packed_floats': 6336, 'sha256': 'dab8fcec1520801c3196bfea08f5567de674128c15f04a834d85a21430c84463'},
    'conv_norm-96-64-1-2-0-0': {'packed_floats': 6336, 'sha256': '7b3c0645dea8140488154a2060739eb11693c0e4c187f2d2fff349e4c2a2f146'},
    'conv_norm-96-64-1-2-0-1': {'packed_floats': 6336, 'sha256': 'e44c95ce01430e23360d73443971861153e17f309ee870f6dc4251f25b945539'},
    'conv_norm-96-64-1-2-1-0': {'packed_floats': 6336, 'sha256': '4680a07dabbcefe89e8c450646e9696bcf01b647c171c706b4e96bf2a09b3553'},
    'conv_norm-96-64-1-2-1-1': {'packed_floats': 6336, 'sha256': 'dab8fcec1520801c3196bfea08f5567de674128c15f04a834d85a21430c84463'},
    'conv_norm-96-64-3-1-0-0': {'packed_floats': 55488, 'sha256': '13d5d237921723d640fd5c6f49b744124861e1c64115b6f229d6b7cac25ad07c'},
    'conv_norm-96-64-3-1-0-1': {'packed_floats': 55488, 'sha256': '75cdbc9e51d1c09c1f1084d9c9d8634c5513e98365fa166251d0b153f3c5a477'},
    'conv_norm-96-64-3-1-1-0': {'packed_floats': 55488, 'sha256': '29f241102a0b0e077b0d759d5b1a8def09b420def9dd91d3893287090319adcf'},
    'conv_norm-96-64-3-1-1-1': {'packed_floats': 55488, 'sha256': 'de4c1de7655101920959bfc21a1260207c0eade44f2ad0e40bb54e47532d1265'},
    'conv_norm-96-64-3-2-0-0': {'packed_floats': 55488, 'sha256': '13d5d237921723d640fd5c6f49b744124861e1c64115b6f229d6b7cac25ad07c'},
    'conv_norm-96-64-3-2-0-1': {'packed_floats': 55488, 'sha256': '75cdbc9e51d1c09c1f1084d9c9d8634c5513e98365fa166251d0b153f3c5a477'},
    'conv_norm-96-64-3-2-1-0': {'packed_floats': 55488, 'sha256': '29f241102a0b0e077b0d759d5b1a8def09b420def9dd91d3893287090319adcf'},
    'conv_norm-96-64-3-2-1-1': {'packed_floats': 55488, 'sha256': 'de4c1de7655101920959bfc21a1260207c0eade44f2ad0e40bb54e47532d1265'},
    'encoder-0-0-bf16x3': {'packed_floats': 1614592, 'sha256': '36058f38e88b842e169229b83a327c36f8a6137e182e04a41cc3591955b09d6c', 'workspace_floats': 66846720},
    'encoder-0-0-fp16x2': {'packed_floats': 1103216, 'sha256': '2287c62cbae513bf77aa139a2c73fe0ef8881c358dee497ad6b473554cb1d8aa', 'workspace_floats': 66846720},
    'encoder-0-0-fp32': {'packed_floats': 1103104, 'sha256': '2d32f23d958d38e98a50abacf6af13078d3e64d591b1d9ed1d8ef4d473e0be7a', 'workspace_floats': 66846720},
    'encoder-0-192-bf16x3': {'packed_floats': 2278528, 'sha256': '2fae8a5e7231c76a0a0cbd082e29a6bb8d924016565a269eab05cd830f90f2ac', 'workspace_floats': 66846720},
    'encoder-0-192-fp16x2': {'packed_floats': 1545976, 'sha256': '342ae5a2eabd17ecefb5bd420b74fb59a6e494132e032814c69ade46886ddc1b', 'workspace_floats': 66846720},
    'encoder-0-192-fp32': {'packed_floats': 1545856, 'sha256': 'd655965820a7d627a7976038dd41d01fdc25a19ac604ab6061fb1433e51616c8', 'workspace_floats': 66846720},
    'encoder-1-0-bf16x3': {'packed_floats': 1614592, 'sha256': 'f537d8b2fb271d2923220e0a0b30b5ced4bc4319adf406b090bd4653dad74a67', 'workspace_floats': 66846720},
    'encoder-1-0-fp16x2': {'packed_floats': 1103216, 'sha256': '797e4528fef0c2b70e9e5e38a1adf57da3c998e67e07fd93e57b743b55822f4c', 'workspace_floats': 66846720},
    'encoder-1-0-fp32': {'packed_floats': 1103104, 'sha256': '473809ddfb16c4f46d807f2cf19f397f343360bf00f0ee4c5a271449c69c5966', 'workspace_floats': 66846720},
    'encoder-1-192-bf16x3': {'packed_floats': 2278528, 'sha256': '6bdcfe5273ea34e78c69d309a1126e135bc9c95a95fb96fe74ac8fe15380a89a', 'workspace_floats': 66846720},
    'encoder-1-192-fp16x2': {'packed_floats': 1545976, 'sha256': '2452512dbcb5a0e321660cf3861995f8f67f3aa5bb2d169721361f38221dd55d', 'workspace_floats': 66846720},
    'encoder-1-192-fp32': {'packed_floats': 1545856, 'sha256': 'e753b212c7a0975c7b11216b8a8502d6e80c5f3bcfd8f6dd9ce4a9f5adc073dc', 'workspace_floats': 66846720},
    'encoder-2-0-bf16x3': {'packed_floats': 1614592, 'sha256': '36058f38e88b842e169229b83a327c36f8a6137e182e04a41cc3591955b09d6c', 'workspace_floats': 66881024},
    'encoder-2-0-fp16x2': {'packed_floats': 1103216, 'sha256': '2287c62cbae513bf77aa139a2c73fe0ef8881c358dee497ad6b473554cb1d8aa', 'workspace_floats': 66881024},
    'encoder-2-0-fp32': {'packed_floats': 1103104, 'sha256': '2d32f23d958d38e98a50abacf6af13078d3e64d591b1d9ed1d8ef4d473e0be7a', 'workspace_floats': 66881024},
    'encoder-2-192-bf16x3': {'packed_floats': 2278528, 'sha256': '2fae8a5e7231c76a0a0cbd082e29a6bb8d924016565a269eab05cd830f90f2ac', 'workspace_floats': 66881024},
    'encoder-2-192-fp16x2': {'packed_floats': 1545976, 'sha256': '342ae5a2eabd17ecefb5bd420b74fb59a6e494132e032814c69ade46886ddc1b', 'workspace_floats': 66881024},
    'encoder-2-192-fp32': {'packed_floats': 1545856, 'sha256': 'd655965820a7d627a7976038dd41d01fdc25a19ac604ab6061fb1433e51616c8', 'workspace_floats': 66881024},
    'loftr-256-8': {'packed_floats': 658176, 'sha256': '59b848073772975dac3aa2a6dc090e05a058e90b2395eff47bc60ce0aa025401', 'workspace_floats': 7541824},
    'update_block-conv_gru-128-128-36-2-576-bf16x3': {'packed_floats': 6129220, 'scale_slots': [-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1], 'sha256': '4d61593e8ce5c23ac929190cbdf6a49b68f2b3af991ec3f09ac26ed19164c9ba', 'workspace_floats': 24879872},
    'update_block-conv_gru-128-128-36-2-576-fp16x2': {'packed_floats': 4101744, 'scale_slots': [-1, 459200, 558212, 853256, 2770836, 3065880, 2770836, 3065880, 3951396, 4101740, 1738252, 2180752, 1738252, 2180752, 3361052, 3508640, 3361052, 3508640], 'sha256': '56dbf7363f6c029e6df6ee361e9bab7d08f0b0e69017a1b88706ccbee5d214e6', 'workspace_floats': 24879872},
    'update_block-conv_gru-128-128-36-2-576-fp32': {'packed_floats': 4101700, 'scale_slots': [-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1], 'sha256': 'ab75c9deee31a37f872f61246b7b9d88a57f89187315cf9314a4bdb799141480', 'workspace_floats': 24879872},
    'update_block-sep_conv-128-128-576-1-144-bf16x3': {'packed_floats': 6603684, 'scale_slots': [-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1], 'sha256': '746202e2584b5fcfff15561c407126e04ae4682d22a14c839aab7de4ad91afbd', 'workspace_floats': 25744896},
    'update_block-sep_conv-128-128-576-1-144-fp16x2': {'packed_floats': 4408300, 'scale_slots': [147712, 590276, 676744, 971788, 2037400, 2201372, 3513136, 3677108, 4366016, 4408296, 1463568, 1709460, 2939304, 3185196, 2365472, 2447524, 3841208, 3923260], 'sha256': '023d5c1045b21a3777b681e0c9227e3c1c9fe47315c66d221c7fe3c7822f567c', 'workspace_floats': 25744896},
    'update_block-sep_conv-128-128-576-1-144-fp32': {'packed_floats': 4424612, 'scale_slots': [-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1], 'sha256': '7bfb990a0ec566c6824b1b8088e634817a7f8ae72036c1ee602cda53a5bae2a2', 'workspace_floats': 25744896},
    'update_block-sep_conv-128-64-36-1-576-bf16x3': {'packed_floats': 5821764, 'scale_slots': [-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1], 'sha256': '47d18b0b4bce173c84dab0fd380e0a42b64ec0d78d8aff48d527e7d39e4f01f9', 'workspace_floats': 24341376},
    'update_block-sep_conv-128-64-36-1-576-fp16x2': {'packed_floats': 3892616, 'scale_slots': [-1, 459200, 545668, 840712, 1783444, 1947416, 3013420, 3177392, 3743420, 3892612, 1250572, 1455504, 2480548, 2685480, 2029596, 2070688, 3259572, 3300664], 'sha256': '18c7b0917d25ec15ba31bbdcae21968a5f8d9324552181f04fe1f26a06906e47', 'workspace_floats': 24341376},
    'update_block-sep_conv-128-64-36-1-576-fp16x2-546': {'packed_floats': 3892560, 'scale_slots': [-1, 459200, -1, -1, -1, 1947396, -1, -1, -1, 3892556, -1, -1, -1, -1, -1, -1, -1, -1], 'sha256': '6a250a2846c0039d082bcb22fa570343c5763ce3273c04048da4769f2615fd81', 'workspace_floats': 24341376},
    'update_block-sep_conv-128-64-36-1-576-fp32': {'packed_floats': 3892548, 'scale_slots': [-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1], 'sha256': 'b0f5905259fb5d9bfed6cbdb2cd6477b7f262205e4c1d971046044b7903b7da4', 'workspace_floats': 24341376},
}


def test_case_list_is_the_pinned_one():
    assert sorted(pins.CASES) == sorted(PINS)
    kinds = {k.split("-")[0] for k in PINS}
    assert kinds == {"update_block", "conv2d", "conv_norm", "encoder", "conv3d", "loftr"}


@pytest.mark.parametrize("case_id", sorted(PINS))
def test_pack_unchanged(case_id):
    assert pins.run_case(case_id) == PINS[case_id]
