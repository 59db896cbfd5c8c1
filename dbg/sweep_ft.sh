for ft in 3 5 8 14; do for r in 1 2; do
echo "FT=$ft 24: $(X265AMD_FRAME_THREADS=$ft timeout 300 python dbg/enc_bench.py 24 2 2>/dev/null | tail -1 | cut -d' ' -f1-6)"
echo "FT=$ft 60: $(X265AMD_FRAME_THREADS=$ft timeout 300 python dbg/enc_clip60.py 2>/dev/null | tail -1| cut -d' ' -f1-6)"
done; done
