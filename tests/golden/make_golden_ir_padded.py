"""Golden vectors of ir-fp (the question injected at g layer 2) on grids with n % 32 != 0, recorded from the REFERENCE itself.

Run in the build container only (make_golden imports the reference's model.py):   python tests/golden/make_golden_ir_padded.py

On these grids the chain path runs on the PADDED j axis (njp = 32 ceil(n / 32) pair rows per (question, i) group), where one
256-row tile may hold rows of two questions.  Recorded with make_golden's recorder:
  G-ir196-b32   B = 32, n = 196 (the 14 x 14 stress grid), light (like G-fp196-b32)
  G-ir196-small B = 2,  n = 196, strided objects, full pair rows and all gradients: tile 171 holds both questions
Writes only these two files."""
import make_golden as mg

if __name__ == "__main__":
    mg.record_rl("G-ir196-b32", "ir-fp", 32, 196, seed=62, light=True)
    mg.record_rl("G-ir196-small", "ir-fp", 2, 196, seed=63, strided=True, full=True, full_grads=True)
